"""GPU parity: HIP fields::Tps fit (Gram, projection, tridiagonalisation / MFMA Cholesky,
through the C ABI) vs the oracle's QR + eigen + GCV restatement on the same stations."""
import numpy as np
import pytest

import fitcheck
from conftest import synth_stations
from oracle import tps as otps

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


@pytest.mark.parametrize("n", [12, 70, 200, 813])
def test_fixed_lambda_cholesky_path(hip, n):
    xy, y = synth_stations(n, 100 + n)
    lam = 3e-3
    want = otps.fit(xy, y, lam=lam)
    got = hip.Tps(xy, y, lambda_=lam)
    assert got.n == n and got.lambda_ == lam
    assert np.array_equal(got.knots, want["knots"])
    assert np.array_equal(got.center, want["center"]) and np.array_equal(got.scale, want["scale"])
    # fp64 tolerance: the SPD system has condition ~ e_max/lambda; 1e-8 on coefficients
    assert _rel(got.c, want["c"]) < 1e-8
    assert _rel(got.d, want["d"]) < 1e-8
    rng = np.random.default_rng(n)
    pts = np.column_stack([rng.uniform(-78, -76, 500), rng.uniform(-7, -5, 500)])
    assert _rel(got.predict(pts), otps.predict_points(want, pts)) < 1e-9


@pytest.mark.parametrize("n,mode", [(12, "fields"), (200, "fields"), (200, "converged"), (259, "fields"), (260, "fields"),
                                    (260, "converged"), (813, "fields")])   # 259 / 260: last size of the single-block tridiagonal path, first of the band path
def test_gcv_path(hip, n, mode):
    xy, y = synth_stations(n, 200 + n)
    want = otps.fit(xy, y, gcv_mode=mode)
    got = hip.Tps(xy, y, gcv_mode=mode)
    # 'fields' mode reproduces the same golden-section trajectory; 'converged' locates a flat
    # minimum, so lambda itself only agrees to ~sqrt(eps)
    assert abs(got.lambda_ - want["lambda"]) / want["lambda"] < (1e-8 if mode == "fields" else 1e-6)
    assert abs(got.eff_df - want["eff_df"]) < 1e-5 * want["eff_df"]
    assert abs(got.gcv - want["gcv"]) < 1e-9 * want["gcv"]
    # compare surfaces at the GPU's lambda so the check is on the solve, not on the flat minimum
    ref = otps.fit(xy, y, lam=got.lambda_)
    assert _rel(got.c, ref["c"]) < 1e-8
    assert _rel(got.d, ref["d"]) < 1e-8
    fitcheck.check(fitcheck.gcv_route(n), xy, y, got.lambda_, got, mode)


@pytest.mark.parametrize("n", [322, 323])     # m = 319: the last 8-column band order; m = 320 = B32_MIN_M: the first band-32
def test_gcv_path_at_the_band32_threshold(hip, n):
    xy, y = synth_stations(n, 200 + n)
    got = hip.Tps(xy, y)
    want = otps.fit(xy, y)
    assert abs(got.lambda_ - want["lambda"]) / want["lambda"] < 1e-8
    ref = otps.fit(xy, y, lam=got.lambda_)
    assert _rel(got.c, ref["c"]) < 1e-8 and _rel(got.d, ref["d"]) < 1e-8
    fitcheck.check(fitcheck.gcv_route(n), xy, y, got.lambda_, got)


def test_replicates_are_collapsed(hip):
    xy, y = synth_stations(150, 7)
    xy2 = np.vstack([xy, xy[:9], xy[3:5]])
    y2 = np.concatenate([y, y[:9] + 0.3, y[3:5] - 0.1])
    want = otps.fit(xy2, y2)
    got = hip.Tps(xy2, y2)
    assert got.n == 150
    assert abs(got.lambda_ - want["lambda"]) / want["lambda"] < 1e-8
    ref = otps.fit(xy2, y2, lam=got.lambda_)
    assert _rel(got.c, ref["c"]) < 1e-8 and _rel(got.d, ref["d"]) < 1e-8


def test_exactly_linear_residual_gives_zero_c(hip):
    """G4 KAT: y exactly linear in (x, y) => c = 0 and the surface is that plane."""
    xy, _ = synth_stations(120, 9)
    y = 2.0 + 0.5 * xy[:, 0] - 0.25 * xy[:, 1]
    got = hip.Tps(xy, y, lambda_=1e-3)
    assert np.abs(got.c).max() < 1e-9
    assert np.abs(got.predict(xy) - y).max() < 1e-9


def test_lambda_to_zero_interpolates(hip):
    xy, y = synth_stations(90, 10)
    got = hip.Tps(xy, y, lambda_=1e-10)
    assert np.abs(got.predict(xy) - y).max() < 1e-5


def test_degenerate_inputs_fail_loudly(hip):
    x = np.linspace(0, 1, 30)
    with pytest.raises(hip.MhsError):  # collinear
        hip.Tps(np.column_stack([x, 2 * x + 1]), np.sin(x))
    with pytest.raises(hip.MhsError):  # <= 3 distinct locations
        hip.Tps(np.array([[0, 0], [1, 0], [0, 1], [0, 0.0]]), np.arange(4.0))
    with pytest.raises(hip.MhsError):  # NaN row
        hip.Tps(np.array([[0, 0], [1, 0], [0, 1], [1, np.nan], [2, 2]]), np.arange(5.0))


def test_fit_then_grid_end_to_end(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 160, 200)
    xy, y = synth_stations(400, 21, g)
    want = otps.fit(xy, y)
    got = hip.Tps(xy, y)
    surf = hip.interpolate(g, got).cpu().numpy()
    ref = otps.predict_grid(otps.fit(xy, y, lam=got.lambda_), g.xmin, g.ymax, g.xres, g.yres, 160, 200)
    assert _rel(surf, ref) < 1e-8
    # and against the oracle's own lambda: 1e-6 is the north-star bound
    ref2 = otps.predict_grid(want, g.xmin, g.ymax, g.xres, g.yres, 160, 200)
    assert _rel(surf, ref2) < 1e-6


def test_large_fit_uses_streaming_panel_path(hip):
    """n > 5 123 stations: the first panels of the band reduction exceed the register-resident
    panel kernel (512 threads x 10 rows) and go through the streaming variant."""
    xy, y = synth_stations(5400, 99)
    got = hip.Tps(xy, y)
    want = otps.fit(xy, y)
    assert abs(got.lambda_ - want["lambda"]) / want["lambda"] < 1e-7
    ref = otps.fit(xy, y, lam=got.lambda_)
    assert _rel(got.c, ref["c"]) < 1e-7 and _rel(got.d, ref["d"]) < 1e-7
    fixed = hip.Tps(xy, y, lambda_=got.lambda_)  # Cholesky route agrees with the band route
    assert _rel(fixed.c, got.c) < 1e-8
    fitcheck.check("gcv-band32", xy, y, got.lambda_, got)
    fitcheck.check("chol", xy, y, got.lambda_, fixed)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [4300, 6100])
def test_legacy_eight_column_route_equals_the_default_route(hip, n, monkeypatch):
    """The 8-column band route (MHS_FIT_LEGACY_BAND=1) is what a fit falls back to when a 32-column panel breaks down, and
    what fits beyond 32 768 stations take.  At these sizes its first panels run the DELAYED update scheme (trailing matrices
    taller than 4 000 rows: groups of 8 panels, one MFMA rank-128 update per group, the symmetric products corrected on the
    fly), then the switch to the eager scheme; n = 6 100 also starts with panels taller than the register-resident kernel.
    On the default route these sizes have panels taller than 4 096 rows (a second batch of split-K partial sums in the
    32-column reduction; round-4 advisor finding: only the benchmarks reached them).  Same lambda, GCV and coefficients to
    rounding, and both equal to the oracle's."""
    xy, y = synth_stations(n, 300 + n)
    fast = hip.Tps(xy, y)
    monkeypatch.setenv("MHS_FIT_LEGACY_BAND", "1")
    legacy = hip.Tps(xy, y)
    monkeypatch.delenv("MHS_FIT_LEGACY_BAND")
    assert abs(legacy.lambda_ - fast.lambda_) < 1e-8 * fast.lambda_
    assert abs(legacy.gcv - fast.gcv) < 1e-9 * fast.gcv
    assert _rel(legacy.c, fast.c) < 1e-8 and _rel(legacy.d, fast.d) < 1e-8
    ref = otps.fit(xy, y, lam=fast.lambda_)
    assert _rel(fast.c, ref["c"]) < 1e-7 and _rel(fast.d, ref["d"]) < 1e-7
    fitcheck.check("gcv-band32", xy, y, fast.lambda_, fast)
    fitcheck.check("gcv-band8", xy, y, legacy.lambda_, legacy, "legacy")


@pytest.mark.parametrize("n", [12, 131, 250])
def test_reduction_cache_refits_are_bit_identical(hip, n):
    """mhs_tps_reduction_cache: a second response on the same stations reuses the reduction (reflectors, tridiagonal,
    projected rows) and sends only its right-hand side through it -- the coefficients, lambda, GCV and effective
    degrees of freedom are those of a full fit, bit for bit; other stations or replicate weights do not hit."""
    from machisplin_amd import tps
    rng = np.random.default_rng(n)
    xy = rng.uniform(0, 1, (n, 2))
    ys = [np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1]) + 0.1 * rng.standard_normal(n) for _ in range(3)]
    full = [hip.Tps(xy, y) for y in ys]
    with tps.reduction_cache():
        cached = [hip.Tps(xy, y) for y in ys]                      # the first builds the entry, the others hit it
        other = hip.Tps(xy[::-1].copy(), ys[0][::-1].copy())        # other order of the stations: another entry
        dup_xy = np.vstack([xy, xy[:3]]); dup_y = np.concatenate([ys[1], ys[1][:3] + 0.2])
        dup = hip.Tps(dup_xy, dup_y)                                # replicates: other weights, no hit
    for a, b in zip(full, cached):
        assert a.lambda_ == b.lambda_ and a.gcv == b.gcv and a.eff_df == b.eff_df
        assert np.array_equal(a.c, b.c) and np.array_equal(a.d, b.d)
    ref = hip.Tps(xy[::-1].copy(), ys[0][::-1].copy())
    assert np.array_equal(other.c, ref.c) and other.lambda_ == ref.lambda_
    ref_dup = hip.Tps(dup_xy, dup_y)
    assert np.array_equal(dup.c, ref_dup.c) and dup.lambda_ == ref_dup.lambda_
    again = hip.Tps(xy, ys[2])                                      # after the scope: a plain fit again
    assert np.array_equal(again.c, full[2].c)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [700, 2211, 4100, 5200])
def test_reduction_cache_band_route_refits_are_bit_identical(hip, n):
    """The same for fits beyond the small route (round 3): the band reduction of Q2'KQ2 -- reduced matrix with its
    reflectors, the panels' T factors and (tau, G) records, the band, the projected rows -- is kept, and another response
    layer on the same stations (V73:203: machisplin.mltps loops over the layers of ONE station table) sends only its
    right-hand side through band_qt_kernel, which repeats every panel's update of g exactly: lambda, GCV, effective
    degrees of freedom, c and d equal the full fit's bit for bit.  n = 700: one to two waves per panel; 2 211: the 1-4
    wave forms and the 8-wave form; 4 100: the delayed scheme's first panels as well.  (Since round 4 these sizes take the
    32-column route and its band32_qt replay; 5 200: panels taller than 4 096 rows -- a second batch of split-K partial sums,
    several chunks per row block -- which only the benchmarks reached before: round-4 advisor finding.)"""
    import time
    from machisplin_amd import tps
    rng = np.random.default_rng(n)
    xy = rng.uniform(0, 1, (n, 2))
    ys = [np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1]) + 0.1 * rng.standard_normal(n) + k * xy[:, 0] for k in range(3)]
    full = [hip.Tps(xy, y) for y in ys]
    with tps.reduction_cache():
        t0 = time.perf_counter(); first = hip.Tps(xy, ys[0]); t1 = time.perf_counter()
        rest = [hip.Tps(xy, y, gcv_mode=mode) for y, mode in ((ys[1], "fields"), (ys[2], "fields"), (ys[1], "converged"))]
        t2 = time.perf_counter()
        fixed = hip.Tps(xy, ys[1], lambda_=1e-3)                     # the Cholesky route never touches the cache
    conv = hip.Tps(xy, ys[1], gcv_mode="converged")
    for a, b in zip(full + [conv], [first] + rest):
        assert a.lambda_ == b.lambda_ and a.gcv == b.gcv and a.eff_df == b.eff_df
        assert np.array_equal(a.c, b.c) and np.array_equal(a.d, b.d)
    assert np.array_equal(fixed.c, hip.Tps(xy, ys[1], lambda_=1e-3).c)
    print("n = %d: first fit (builds the entry) %.1f ms, later layers %.1f ms each" % (n, (t1 - t0) * 1e3, (t2 - t1) * 1e3 / 3))


@pytest.mark.timeout(600)
def test_breakdown_of_the_32_column_route_falls_back_and_is_remembered(hip, monkeypatch, capfd):
    """Stations in near-coincident pairs (1e-9 of the range apart: distinct cells for the replicate collapse, identical rows
    for the Gram matrix) make a panel of the 32-column Cholesky-QR numerically rank deficient: the fit must hand itself back to
    the 8-column Householder route -- same lambda and coefficients as MHS_FIT_LEGACY_BAND=1 gives, bit for bit (it IS that
    route, on a rebuilt matrix) -- and, inside a reduction-cache scope, remember the verdict: the other response layers go
    straight to the 8-column route (round-4 advisor finding: they repeated the failing reduction), with the fresh fits' bits."""
    from machisplin_amd import tps
    rng = np.random.default_rng(77)
    base = rng.uniform(0, 1, (330, 2))
    xy = np.vstack([base, base + 1e-9 * rng.standard_normal(base.shape)])
    ys = [np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1]) + 0.1 * rng.standard_normal(len(xy)) + k * xy[:, 1] for k in range(2)]
    monkeypatch.setenv("MHS_TIMING", "1")
    capfd.readouterr()
    got = hip.Tps(xy, ys[0])
    err = capfd.readouterr().err
    assert "handed the fit back" in err, "the station set did not break the 32-column route: the test exercises nothing"
    with tps.reduction_cache():
        first = hip.Tps(xy, ys[0])
        capfd.readouterr()
        second = hip.Tps(xy, ys[1])
        err2 = capfd.readouterr().err
    assert "handed the fit back" not in err2 and "32-column" not in err2      # no second attempt
    monkeypatch.delenv("MHS_TIMING")
    monkeypatch.setenv("MHS_FIT_LEGACY_BAND", "1")
    legacy = [hip.Tps(xy, y) for y in ys]
    monkeypatch.delenv("MHS_FIT_LEGACY_BAND")
    for a, b in ((got, legacy[0]), (first, legacy[0]), (second, legacy[1])):
        assert a.lambda_ == b.lambda_ and np.array_equal(a.c, b.c) and np.array_equal(a.d, b.d)
    ref = otps.fit(xy, ys[0], lam=got.lambda_)
    assert _rel(got.d, ref["d"]) < 1e-6
