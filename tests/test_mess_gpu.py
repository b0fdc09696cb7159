"""GPU: the MESS extrapolation map (csrc/mess.hip, machisplin_amd/mess.py) against the numpy restatement of the rule
(tests/mess_ref.py).  The MESS plane must equal the restatement bit for bit (NaN where it is NaN) and the MoD plane exactly:
the library is built without contraction and the rule fixes the order of the operations, so there is no tolerance.

Grids are 150 x 197 cells (29 chunks of 1 024 cells: several blocks, chunks that run over row ends, a partly filled last
chunk).  Every case plants, at known cells, values equal to a reference value, to the variable's min, to its max, below the
min and above the max.  Reference sizes 2, 3, 63, 64, 65, 129 and 732 sit around the 64-value segments of the kernel's
two-level search; 37 312 and 37 313 rows x 7 variables sit on either side of the size at which the coarse table no longer
goes to LDS (V (ceil(n / 64) + 2) <= 4 096 doubles)."""
import functools

import numpy as np
import pytest

import mess_ref

pytestmark = pytest.mark.gpu

NODATA = -32768.0
NROW, NCOL = 150, 197
WINDOW = (7, 68, 13, 96)          # r0, c0 != 0; 61 x 83 cells: no multiple of 64, 16 or 4

#        dtype, n_ref, C, V
CASES = [("f64", 2, 5, 5), ("f64", 63, 5, 7), ("f64", 732, 1, 1), ("f64", 129, 1, 3),
         ("f32", 3, 5, 7), ("f32", 64, 5, 5), ("f32", 129, 1, 1), ("f32", 37312, 5, 7),
         ("i16", 65, 5, 5), ("i16", 732, 5, 7), ("i16", 2, 1, 1), ("i16", 37313, 5, 7)]
IDS = [f"{d}-n{n}-C{c}-V{v}" for d, n, c, v in CASES]


def _geom():
    from machisplin_amd import synth
    return synth.grid(NROW, NCOL)


@functools.lru_cache(maxsize=None)
def _case(dtype, n_ref, C, V):
    """planes (numpy, the plane dtype), the reference table, the planted cells and the restatement's planes: built once"""
    seed = n_ref * 31 + C * 7 + V + {"f64": 0, "f32": 1, "i16": 2}[dtype]
    rng = np.random.default_rng(seed)
    g = _geom()
    np_dt = {"f64": np.float64, "f32": np.float32, "i16": np.int16}[dtype]
    if dtype == "i16":
        planes = rng.integers(-200, 1200, size=(C, NROW, NCOL)).astype(np.int16)
    else:
        planes = (rng.standard_normal((C, NROW, NCOL)) * 300.0 + 500.0).astype(np_dt)
    # the reference rows: the variables at sampled cells (so that cell values EQUAL reference values), taken from the
    # middle of the grid only (cells outside it then fall below the min / above the max of LONG and LAT), rows repeated
    while True:
        rr = rng.integers(20, NROW - 20, size=n_ref)
        cc = rng.integers(25, NCOL - 25, size=n_ref)
        if n_ref >= 3:
            rr[1], cc[1] = rr[0], cc[0]                      # a duplicated row: duplicated values in every variable
        ref = np.column_stack([planes[k, rr, cc].astype(np.float64) for k in range(C)] +
                              [g.x_from_col(cc), g.y_from_row(rr)])[:, :V]
        if (ref.max(0) > ref.min(0)).all():
            break
    srt = np.sort(ref, axis=0)
    # planted cells (layer 0): equal to the min, the max, a middle reference value, below the min, above the max
    delta = 3 if dtype == "i16" else 0.75
    planted = {"min": ((3, 5), srt[0, 0]), "max": ((3, 70), srt[-1, 0]), "mid": ((90, 5), srt[n_ref // 2, 0]),
               "below": ((149, 196), srt[0, 0] - delta), "above": ((0, 0), srt[-1, 0] + delta),
               "win_max": ((WINDOW[0], WINDOW[2]), srt[-1, 0]), "win_below": ((WINDOW[1] - 1, WINDOW[3] - 1), srt[0, 0] - delta)}
    planted = {name: (cell, float(np_dt(val))) for name, (cell, val) in planted.items()}     # as the plane type holds it
    assert planted["below"][1] < srt[0, 0] and planted["win_below"][1] < srt[0, 0] and planted["above"][1] > srt[-1, 0]
    for (r, c), val in planted.values():
        planes[0, r, c] = np_dt(val)
    # NA cells: the stack's nodata everywhere, NaN too in float planes
    k = rng.integers(0, C, size=400); r = rng.integers(0, NROW, size=400); c = rng.integers(0, NCOL, size=400)
    free = np.ones((NROW, NCOL), dtype=bool)
    for (pr, pc), _ in planted.values():
        free[pr, pc] = False
    ok = free[r, c]
    planes[k[ok][:200], r[ok][:200], c[ok][:200]] = np_dt(NODATA)
    if dtype != "i16":
        planes[k[ok][200:], r[ok][200:], c[ok][200:]] = np.nan
    want, want_mod = mess_ref.mess(ref, mess_ref.grid_values(g, planes, NODATA, V))
    return g, planes, ref, planted, want, want_mod


@functools.lru_cache(maxsize=None)
def _device(dtype, n_ref, C, V):
    import machisplin_amd as hip
    g, planes, ref, planted, want, want_mod = _case(dtype, n_ref, C, V)
    stack = hip.RasterStack(g, planes, NODATA)
    m = hip.Mess(ref)
    got, mod = m.grid(stack, mod=True)
    return stack, m, got.cpu().numpy(), mod.cpu().numpy()


@pytest.mark.parametrize("dtype,n_ref,C,V", CASES, ids=IDS)
def test_grid_planes_equal_the_restatement_bit_for_bit(hip, dtype, n_ref, C, V):
    g, planes, ref, planted, want, want_mod = _case(dtype, n_ref, C, V)
    stack, m, got, mod = _device(dtype, n_ref, C, V)
    assert (m.n_ref, m.n_vars) == (n_ref, V)
    assert got.dtype == np.float64 and mod.dtype == np.int32
    # the planted cases are what they claim to be (the restatement's own count), and NA cells exist
    srt0 = np.sort(ref[:, 0])
    count = {name: int(np.searchsorted(srt0, val, side="right")) for name, (_, val) in planted.items()}
    assert count["below"] == 0 and count["win_below"] == 0 and count["above"] == n_ref and count["max"] == n_ref and count["win_max"] == n_ref
    assert 0 < count["min"] and 0 < count["mid"] and (count["mid"] < n_ref or n_ref == 2)
    assert mess_ref.similarity(ref[:, 0], np.array([planted["max"][1]]))[0] == 0.0          # the i == n quirk
    for name in ("below", "above", "win_below"):
        (r, c), _ = planted[name]
        assert want[r, c] < 0.0 and got[r, c] < 0.0
    na = np.isnan(want)
    assert na.any() and (want_mod[na] == -1).all() and not na.all()
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(mod, want_mod)


@pytest.mark.parametrize("dtype,n_ref,C,V", CASES, ids=IDS)
def test_window_no_mod_points_and_repeat(hip, dtype, n_ref, C, V):
    import torch
    g, planes, ref, planted, want, want_mod = _case(dtype, n_ref, C, V)
    stack, m, got, mod = _device(dtype, n_ref, C, V)
    r0, r1, c0, c1 = WINDOW
    # a window into a wider buffer (ld > ncol of the window) equals the same cells of the whole-grid plane
    big = torch.full((r1 - r0, 100), -7.0, dtype=torch.float64, device=stack.planes.device)
    bigm = torch.full((r1 - r0, 111), -7, dtype=torch.int32, device=stack.planes.device)
    w, wm = m.grid(stack, window=WINDOW, out=big[:, :c1 - c0], mod=bigm[:, :c1 - c0])
    assert w.stride(0) == 100 and wm.stride(0) == 111
    assert np.array_equal(w.cpu().numpy(), got[r0:r1, c0:c1], equal_nan=True)
    assert np.array_equal(wm.cpu().numpy(), mod[r0:r1, c0:c1])
    assert (big[:, c1 - c0:] == -7.0).all() and (bigm[:, c1 - c0:] == -7).all()          # nothing written beside the window
    # without the MoD plane: the same MESS plane; a second call: the same bits
    alone = m.grid(stack)
    assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), got, equal_nan=True)
    again, again_mod = m.grid(stack, mod=True)
    assert np.array_equal(again.cpu().numpy(), got, equal_nan=True) and np.array_equal(again_mod.cpu().numpy(), mod)
    # the points call on the cells' own values (LONG / LAT columns included) equals the grid plane
    vals = mess_ref.grid_values(g, planes, NODATA, V)
    X = np.column_stack([np.asarray(v).ravel() for v in vals])
    pm, pv = m.points(X)
    assert pm.dtype == np.float64 and pv.dtype == np.int32
    assert np.array_equal(pm.reshape(NROW, NCOL), got, equal_nan=True)
    assert np.array_equal(pv.reshape(NROW, NCOL), mod)


def test_more_chunks_than_blocks(hip):
    """1 100 chunks of 1 024 rows: more than the 4 blocks per compute unit the launch is capped at, so blocks take
    several chunks (the grid-stride loop no 150 x 197 grid reaches)."""
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((200, 1))
    X = rng.standard_normal((1100 * 1024 - 37, 1)) * 1.5
    X[::1001] = np.nan
    m = hip.Mess(ref)
    got, mod = m.points(X)
    want, want_mod = mess_ref.mess(ref, [X[:, 0]])
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(mod, want_mod)


def test_grid_refuses_a_table_that_does_not_fit_the_stack(hip):
    g, planes, ref, *_ = _case("f32", 64, 5, 5)
    stack = hip.RasterStack(g, planes, NODATA)
    for V in (4, 6, 8):
        m = hip.Mess(np.random.default_rng(V).standard_normal((10, V)))
        with pytest.raises(hip.MhsError) as ei:
            m.grid(stack)
        assert ei.value.code == hip._lib.ERR_INVALID and "two more" in str(ei.value)


def _same(a, b):
    import torch
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b or (a != a and b != b)


def test_mltps_predict_mess_option(hip):
    from machisplin_amd import mltps, synth
    g = _geom()
    planes, nodata = synth.covariates(g, 3, 17, dtype="i16", nodata_frac=0.02)
    stack = hip.RasterStack(g, planes, nodata)
    xy, rows, cols, uv = synth.stations(g, 220, 17)
    X, _, _ = mltps.station_predictors(stack, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert 0 < (~keep).sum() < 60                                   # some stations sit on nodata cells and are dropped
    resp = synth.response(np.nan_to_num(X), uv, 17)
    models = [hip.models.from_param_dict(p) for p in synth.ensemble_params(X[keep], resp[keep], 17, which="g")]
    base = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None)
    off = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=False)
    assert "mess" not in base and "mess_var" not in base and _same(base, off)
    for flag, table in ((True, X[keep][:, :3]), ("all", X[keep])):
        res = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=flag)
        want, want_mod = hip.Mess(table).grid(stack, mod=True)
        assert np.array_equal(res["mess"].cpu().numpy(), want.cpu().numpy(), equal_nan=True)
        assert np.array_equal(res["mess_var"].cpu().numpy(), want_mod.cpu().numpy())
        ref_m, ref_v = mess_ref.mess(table, mess_ref.grid_values(g, planes.cpu().numpy(), nodata, table.shape[1]))
        assert np.array_equal(res["mess"].cpu().numpy(), ref_m, equal_nan=True) and np.array_equal(res["mess_var"].cpu().numpy(), ref_v)
        assert _same({k: v for k, v in res.items() if k not in ("mess", "mess_var")}, base)
    # the layer loop passes the option on
    omega = hip.mltps_layers(stack, np.column_stack([xy, resp]), [{"models": models, "weights": [1.0], "wt_total": 1.0}],
                             tile_edge=None, mess=True)
    assert np.array_equal(omega[0]["mess"].cpu().numpy(), hip.Mess(X[keep][:, :3]).grid(stack).cpu().numpy(), equal_nan=True)
    assert "mess" not in hip.mltps_layers(stack, np.column_stack([xy, resp]), [{"models": models, "weights": [1.0], "wt_total": 1.0}],
                                          tile_edge=None)[0]
