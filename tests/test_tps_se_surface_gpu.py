"""GPU: the SE plane of the tiled Step 3 + 4 (mhs_tps_surface_se_dev) against its composition from the public pieces --
per-tile interpolate_se of the tile's fit_many spline on its keep window (NaN for a zero tile), then the mosaic and
seam feathering of tiles.mosaic_feather -- and the one-tile / global cases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _stations(g, n, seed, empty_box=None):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, g.nrow, 4 * n)
    cols = rng.integers(0, g.ncol, 4 * n)
    if empty_box is not None:
        r0, r1, c0, c1 = empty_box
        keep = ~((rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1))
        rows, cols = rows[keep], cols[keep]
    cell = rng.permutation(np.unique(rows * g.ncol + cols))[:n]
    rows, cols = np.divmod(cell, g.ncol)
    xy = np.column_stack([g.x_from_col(cols), g.y_from_row(rows)])
    u = (xy - xy.min(0)) / (xy.max(0) - xy.min(0))
    y = np.sin(5 * u[:, 0]) * np.cos(4 * u[:, 1]) + 0.1 * rng.standard_normal(xy.shape[0])
    return xy, y


def _composed(hip, g, xy, y, tile_edge, cov1=None):
    nRx, nCx, fit_win, keep_win = hip.tiles.step3_tile_windows(g, tile_edge)
    rows, cols = hip.tiles.cells_from_xy(g, xy)
    ok = rows >= 0
    if cov1 is not None:
        ok &= ~np.isnan(cov1)
    sels = [np.flatnonzero(ok & (rows >= f[0]) & (rows < f[1]) & (cols >= f[2]) & (cols < f[3])) for f in fit_win]
    todo = [h for h in range(nRx * nCx) if sels[h].size >= 10]
    fits = dict(zip(todo, hip.tps.fit_many([xy[sels[h]] for h in todo], [y[sels[h]] for h in todo])))
    bufs = []
    for h in range(nRx * nCx):
        fr0, fr1, fc0, fc1 = (int(v) for v in fit_win[h])
        kr0, kr1, kc0, kc1 = (int(v) for v in keep_win[h])
        if h not in fits:
            bufs.append(torch.full((kr1 - kr0, kc1 - kc0), float("nan"), dtype=torch.float64, device="cuda"))
            continue
        gf = g.window(fr0, fr1, fc0, fc1)
        bufs.append(hip.interpolate_se(gf, fits[h], window=(kr0 - fr0, kr1 - fr0, kc0 - fc0, kc1 - fc0)))
    out = hip.tiles.mosaic_feather(g, nRx, nCx, keep_win, bufs, merge_mode=False)
    return out, nRx, nCx, fit_win, keep_win, sels


def test_tiled_se_surface_equals_the_composition(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 260, 300)
    xy, y = _stations(g, 600, 11)
    got = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=100).cpu().numpy()
    want, nRx, nCx, *_ = _composed(hip, g, xy, y, 100)
    assert nRx * nCx == 9
    want = want.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)


def test_zero_tile_gives_nan_exactly_where_only_it_covers(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 240, 240)
    # no station in the north-west tile's fit box
    xy, y = _stations(g, 500, 12, empty_box=(0, 100, 0, 100))
    got = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=80).cpu().numpy()
    want, nRx, nCx, fit_win, keep_win, sels = _composed(hip, g, xy, y, 80)
    want = want.cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    zero = [h for h in range(nRx * nCx) if sels[h].size < 10]
    assert zero
    covered = np.zeros(got.shape, bool)
    for h in range(nRx * nCx):
        if h not in zero:
            r0, r1, c0, c1 = keep_win[h]
            covered[r0:r1, c0:c1] = True
    assert np.array_equal(np.isnan(got), ~covered)


def test_single_tile_is_the_global_fit(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 90, 110)
    xy, y = _stations(g, 150, 13)
    fit = hip.Tps(xy, y)
    want = hip.interpolate_se(g, fit).cpu().numpy()
    for te in (1500, 0):
        got = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=te or None).cpu().numpy()
        assert np.array_equal(got, want)


def test_estimate_plane_unchanged_by_an_se_call(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 200, 220)
    xy, y = _stations(g, 400, 14)
    before = hip.tps_residual_surface(g, xy, y, tile_edge=80).cpu().numpy()
    se = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=80).cpu().numpy()
    after = hip.tps_residual_surface(g, xy, y, tile_edge=80).cpu().numpy()
    assert np.isfinite(se).all()
    assert np.array_equal(before, after)


def test_tiled_se_surface_drops_stations_on_na_covariate_cells(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 200, 220)
    xy, y = _stations(g, 400, 15)
    cov1 = np.ones(xy.shape[0])
    cov1[::37] = np.nan
    got = hip.mltps.tps_residual_surface_se(g, xy, y, cov1_at_stations=cov1, tile_edge=80).cpu().numpy()
    want, nRx, nCx, fit_win, keep_win, sels = _composed(hip, g, xy, y, 80, cov1=cov1)
    assert nRx * nCx == 9
    assert min(s.size for s in sels) >= 10      # no zero tile: every tile's spline is compared
    assert not np.isnan(cov1[np.concatenate(sels)]).any()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want.cpu().numpy())


def test_nan_residual_station_equals_its_removal(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 200, 220)
    xy, y = _stations(g, 400, 15)
    y = y.copy()
    y[::41] = np.nan
    keep = ~np.isnan(y)
    for surface in (hip.tps_residual_surface, hip.mltps.tps_residual_surface_se):
        got = surface(g, xy, y, tile_edge=80).cpu().numpy()
        want = surface(g, xy[keep], y[keep], tile_edge=80).cpu().numpy()
        assert np.isfinite(want).all()
        assert np.array_equal(got, want)
