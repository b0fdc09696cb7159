"""GPU: every supported predictor count p (covariate layers + LONG + LAT) through the six members.

p is the axis on which the library compiles the most distinct code -- nnet_kernel<P>, small_members_kernel<P>, svr_kernel<P, 3>
and svr_rt_kernel<P, 3> for P = 2 .. 12 (MHS_DISPATCH_P, csrc/ensemble.hip) -- and on which the tree members change route
(gbm: register LUT up to LUT_REG_P = 8, LDS-key LUT up to p = 33, node walk beyond; the forest: the kernels with the
wave-uniform prefix up to RF_PREFIX_MAX_P = 12, the split-node kernel up to p = 15, the double-buffered kernel while its keys fit,
the node walk beyond; the loaders stop at 64).  The reference is always the oracle (oracle/ensemble.py) on the same planes, the
tolerance the project's 1e-11 * max |ref|, NaN patterns equal.  Models are small: 150 stations, 20 gbm trees, 3 forest trees.

A stack without covariate layers cannot be expressed (RasterStack has no planes to point at, and mhs_predict_dev refuses a NULL
stack), so P = 2 is reached through predict_points alone.

Which kernel ran: the ksvm row-tile kernel and gbm's coherent kernel sum in another order than their lane-per-cell / tree-order
siblings, so planes that differ in their last bits prove them; every other tree kernel gives the node walk's bits BY DESIGN, so
for those a forcing variable (MHS_RF_KERNEL, MHS_GBM_NO_COHERENT, MHS_TREES_GENERIC) is all the evidence there is -- the tests
below run every forcing on both sides of every boundary and say in their docstrings what launch_forest / launch_gbm_lut select
there by the conditions in the code.  In particular nothing outside the library can tell gbm_lut_kernel (p = 9) from the
node walk; what the p = 9 case does show is that the register kernels of p = 8 no longer run."""
import numpy as np
import pytest

from oracle import ensemble as oe
from oracle import tps as otps

pytestmark = pytest.mark.gpu

KINDS = "bgnmrv"
DTYPES = ("f32", "f64", "i16")
WTS = {"g": 0.22, "n": 0.12, "m": 0.18}
_CACHE = {}


def _tol(ref):
    return 1e-11 * np.nanmax(np.abs(ref))


def _setup(hip, C, dtype=None, nrow=9, ncol=190, crop=None, n=150, seed=5, nodata_frac=0.01):
    """Planes of C layers on an nrow x ncol grid, 150 stations on its cells, the six members fitted to them.  `crop` = (r, c):
    the stack handed to the library is the grid's north-west r x c corner (same origin and cell size: the same cell centres), with
    one NoData cell put inside it.  Cached: the tests share the models of a p."""
    import torch
    from machisplin_amd import synth
    key = (C, dtype, nrow, ncol, crop, n, seed)
    if key in _CACHE:
        return _CACHE[key]
    dtype = dtype or DTYPES[(C + 2) % 3]
    g = synth.grid(nrow, ncol)
    planes, nodata = synth.covariates(g, C, seed, dtype=dtype, nodata_frac=nodata_frac)
    if crop:
        planes[:, 2, 3] = -32768 if dtype == "i16" else float("nan")
    host = planes.cpu().numpy().astype(np.float64)
    if not np.isnan(nodata):
        host[host == nodata] = np.nan
    x, y = otps.cell_centres(g.xmin, g.ymax, g.xres, g.yres, nrow, ncol)
    X = oe.stack_predictors(host, (x, y))
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(~np.isnan(X).any(axis=1))
    idx = rng.choice(ok, n, replace=False)
    Xs = X[idx]
    uv = np.column_stack([(idx % ncol + 0.5) / ncol, (idx // ncol + 0.5) / nrow])
    ys = synth.response(Xs, uv, seed)
    params = synth.ensemble_params(Xs, ys, seed, n_gbm_trees=20, n_rf_trees=3)
    if crop:
        r, c = crop
        g = synth.grid(r, c)
        planes = planes[:, :r, :c].contiguous()
        x, y = otps.cell_centres(g.xmin, g.ymax, g.xres, g.yres, r, c)
        X = oe.stack_predictors(host[:, :r, :c], (x, y))
    out = {"g": g, "stack": hip.RasterStack(g, planes, nodata), "X": X, "Xs": Xs, "ys": ys, "params": dict(zip(KINDS, params)),
           "dtype": dtype, "torch": torch}
    _CACHE[key] = out
    return out


def _check(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.nanmax(np.abs(got - want))
    assert err <= _tol(want), (what, err, _tol(want))


def _same_bits(a, b, what):
    import torch
    assert torch.equal(torch.isnan(a), torch.isnan(b)), what
    assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), what


def _with_env(monkeypatch, envs, fn):
    for e, v in envs.items():
        monkeypatch.setenv(e, v)
    try:
        return fn()
    finally:
        for e in envs:
            monkeypatch.delenv(e)


# ------------------------------------------------------------------------------------------ grid mode, p = 3 .. 12 --
@pytest.mark.parametrize("p", range(3, 13))
def test_all_six_members_on_a_grid(hip, p, monkeypatch):
    """C = 1 .. 10 layers, the plane type rotating with p, 1 % NoData, 9 x 190 cells: one ragged 192-cell row tile per row, which
    satisfies nc >= 0.93 * tpr * 192, so ksvm takes svr_rt_kernel<P, 3>; a 100-column window does not, and takes svr_kernel<P, 3>
    in grid mode.  ksvm: both planes against the oracle, against each other to 1e-12 (the row-tile kernel folds the wave's
    largest exponent and scales back, so the two agree to rounding and NOT bitwise: that they differ is the proof that it ran),
    and the window bit for bit the slice of the lane-per-cell plane."""
    s = _setup(hip, p - 2)
    assert s["dtype"] == DTYPES[p % 3] and np.isnan(s["X"]).any()
    for k in "bgnmr":
        prm = s["params"][k]
        got = hip.predict(s["stack"], hip.models.from_param_dict(prm)).cpu().numpy()
        _check(got, oe.predict(prm, s["X"]), (p, prm["kind"]))
    prm = s["params"]["v"]
    assert (prm["alpha"] > 0).any() and (prm["alpha"] < 0).any()
    m = hip.models.from_param_dict(prm)
    want = oe.predict(prm, s["X"])
    rowtile = hip.predict(s["stack"], m).cpu().numpy()
    window = hip.predict(s["stack"], m, window=(0, 9, 45, 145)).cpu().numpy()
    plain = _with_env(monkeypatch, {"MHS_SVR_NO_ROWTILE": "1"}, lambda: hip.predict(s["stack"], m)).cpu().numpy()
    _check(rowtile, want, (p, "svr_rt_kernel"))
    _check(plain, want, (p, "svr_kernel"))
    assert np.nanmax(np.abs(rowtile - plain)) <= 1e-12 * np.nanmax(np.abs(plain))
    assert not np.array_equal(rowtile, plain, equal_nan=True), "the row-tile kernel did not run (identical planes)"
    assert np.array_equal(window, plain[:, 45:145], equal_nan=True)


# ---------------------------------------------------------------------------------------- points mode, p = 2 .. 12 --
@pytest.mark.parametrize("p", range(2, 13))
def test_nnet_and_ksvm_on_points(hip, p):
    """predict_points (the stations' residual inputs): nnet_kernel<P> and svr_kernel<P, 3> on a table of n x p columns; p = 2 is
    LONG and LAT alone."""
    from machisplin_amd import synth
    s = _setup(hip, max(p - 2, 1))
    Xs = s["Xs"] if p > 2 else s["Xs"][:, -2:]
    for prm in (synth.nnet_params(Xs, s["ys"], 40 + p), synth.svr_params(Xs, s["ys"], 40 + p)):
        m = hip.models.from_param_dict(prm)
        assert m.p == p
        want = oe.predict(prm, Xs)
        got = m.predict_points(Xs)
        assert np.abs(got - want).max() <= _tol(want), (p, prm["kind"])
        assert np.array_equal(m.predict_points(Xs[:1]), got[:1]) and np.array_equal(m.predict_points(Xs[:65])[64:], got[64:65])


# ------------------------------------------------------------------------------- fused small members, p = 3 .. 12 --
def _fused_runs(hip, s, subsets, what):
    for which in subsets:
        sel = [s["params"][k] for k in which]
        mods = [hip.models.from_param_dict(q) for q in sel]
        wts = [WTS[k] for k in which]
        fused = hip.models.members_predict(s["stack"], mods, wts)
        acc = hip.predict(s["stack"], mods[0], weight=wts[0])
        for m, w in zip(mods[1:], wts[1:]):
            hip.predict(s["stack"], m, weight=w, accumulate=True, out=acc)
        _same_bits(fused, acc, (what, which))
        want = None
        for q, w in zip(sel, wts):
            pk = oe.predict(q, s["X"]) * w
            want = pk if want is None else want + pk
        _check(fused.cpu().numpy(), want, (what, which))


@pytest.mark.parametrize("p", range(3, 13))
def test_fused_small_members(hip, p):
    """small_members_kernel<P>: the runs lm+nnet+earth, lm+nnet, nnet+earth and lm+earth of mhs_members_predict_dev in one pass --
    the bits of member-by-member accumulation, and the oracle's weighted sum."""
    _fused_runs(hip, _setup(hip, p - 2), ("gnm", "gn", "nm", "gm"), p)


@pytest.mark.parametrize("p", [13, 64])
def test_small_members_beyond_the_fused_kernel(hip, p):
    """p > PMAX = 12: launch_members fuses nothing, lm and earth run one after the other -- same two criteria"""
    _fused_runs(hip, _setup(hip, p - 2, nrow=30, ncol=40, crop=(5, 7), nodata_frac=0.05), ("gm",), p)


# --------------------------------------------------------------------------------------------- p in {13, 33, 64} --
def _use_last_covariate_and_lat(s, p):
    """at least one earth factor, one gbm split and one forest split on the last covariate (predictor p - 3) and on LAT (p - 1)"""
    Xs = s["Xs"]
    earth, gbm, rf = s["params"]["m"], s["params"]["b"], s["params"]["r"]
    for term, v in ((1, p - 3), (2, p - 1)):
        earth["dirs"][term, :] = 0
        earth["cuts"][term, :] = 0.0
        earth["dirs"][term, v], earth["cuts"][term, v] = (1, -1)[term - 1], np.median(Xs[:, v])
    for tree, v in ((0, p - 3), (1, p - 1)):
        root = gbm["tree_offsets"][tree]
        assert gbm["split_var"][root] >= 0
        gbm["split_var"][root], gbm["split_val"][root] = v, np.median(Xs[:, v])
        root = rf["tree_offsets"][tree]
        assert rf["status"][root] == -3
        rf["best_var"][root], rf["split"][root] = v + 1, np.median(Xs[:, v])


@pytest.mark.parametrize("p", [13, 33, 40, 41, 64])
def test_lm_earth_gbm_and_forest_with_many_predictors(hip, p, monkeypatch):
    """The members without a compiled-in P, beyond the twelve of the register kernels: p = 13, p = 33 (the last p whose keys fit
    beside gbm's LUT chunk: 33 * 4 096 + 16 384 <= LDS_LIMIT) and p = 64 (the loaders' limit; gbm and the forest take the node
    walk), on points and on a 5 x 7 grid with a NoData cell.  The tree members' planes are the node walk's bit for bit.

    p = 64 is the regression test of a failure this test found: the node walk parks the predictors of two cells per lane in
    LDS, 4 096 p bytes, which no longer fits the 160 KiB of a compute unit from p = 41 on -- every gbm and forest model of
    41 .. 64 predictors loaded and then failed in predict (hipFuncSetAttribute: invalid argument), on grids and on points, and
    left the error for the next user of the runtime to find.  Such models now walk one cell per lane; p = 40 | 41 is that
    boundary."""
    s = _setup(hip, p - 2, nrow=30, ncol=40, crop=(5, 7), nodata_frac=0.05)
    if not s.get("patched"):
        _use_last_covariate_and_lat(s, p)
        s["patched"] = True
    earth, gbm, rf = s["params"]["m"], s["params"]["b"], s["params"]["r"]
    for v in (p - 3, p - 1):
        assert (earth["dirs"][:, v] != 0).any() and (gbm["split_var"] == v).any()
        assert (rf["best_var"][rf["status"] == -3] == v + 1).any()
    assert np.isnan(s["X"]).any()
    for k in "gmbr":
        prm = s["params"][k]
        m = hip.models.from_param_dict(prm)
        want = oe.predict(prm, s["X"])
        grid = hip.predict(s["stack"], m)
        _check(grid.cpu().numpy(), want, (p, prm["kind"], "grid"))
        pts = m.predict_points(s["Xs"])
        ref = oe.predict(prm, s["Xs"])
        assert np.abs(pts - ref).max() <= _tol(ref), (p, prm["kind"], "points")
        if k in "br":
            walk = _with_env(monkeypatch, {"MHS_TREES_GENERIC": "1"}, lambda: hip.predict(s["stack"], m))
            _same_bits(grid, walk, (p, prm["kind"]))


# ------------------------------------------------------------------------------------------------ route boundaries --
@pytest.mark.parametrize("p,nrow,ncol", [(8, 20, 48), (9, 20, 48), (8, 9, 250), (9, 9, 250)])
def test_gbm_register_lut_boundary(hip, p, nrow, ncol, monkeypatch):
    """LUT_REG_P = 8.  60 five-split trees (lut_S = 5; not a multiple of the 64-tree chunk).
    p = 8: the keys live in registers.  By default the window takes gbm_coherent_kernel (nr >= 8, nc >= 0.8 x its 16-column tiles;
    below 2^20 cells no probe), whose sum runs in another order: its plane differs from the tree-order plane
    (MHS_GBM_NO_COHERENT=1: gbm_lutreg_kernel on 48 columns, gbm_lutreg_rt_kernel on 250 = one ragged 256-cell row tile) in the
    last bits -- the proof that the register route was taken -- and equals MHS_GBM_FORCE_COHERENT=1 bit for bit.
    p = 9: neither register kernel applies (in_regs is false), the forcing variables change nothing, and the plane is the node
    walk's whichever of gbm_lut_kernel<5> (what launch_gbm_lut selects: 9 * 4 096 + 16 384 bytes of LDS) and the node walk ran.
    Every plane is the node walk's to rounding (1e-13, the project's number for the coherent order) and the oracle's."""
    from machisplin_amd import synth
    s = _setup(hip, p - 2, dtype="f32", nrow=nrow, ncol=ncol)
    prm = synth.gbm_params(s["Xs"], s["ys"], 3, n_trees=60)
    assert set(np.unique(prm["split_var"][prm["split_var"] >= 0])) == set(range(p))          # every predictor splits, LAT included
    m = hip.models.from_param_dict(prm)
    default = hip.predict(s["stack"], m)
    ordered = _with_env(monkeypatch, {"MHS_GBM_NO_COHERENT": "1"}, lambda: hip.predict(s["stack"], m))
    forced = _with_env(monkeypatch, {"MHS_GBM_FORCE_COHERENT": "1"}, lambda: hip.predict(s["stack"], m))
    walk = _with_env(monkeypatch, {"MHS_TREES_GENERIC": "1"}, lambda: hip.predict(s["stack"], m))
    torch = s["torch"]
    assert not torch.isnan(default).any()                  # gbm routes NA covariates through its MissingNode children
    _same_bits(ordered, walk, (p, "tree order"))
    _same_bits(default, forced, (p, "forced coherent"))
    assert float((default - walk).abs().max()) <= 1e-13 * float(walk.abs().max())
    if p <= 8:
        assert not torch.equal(default, ordered), "gbm_coherent_kernel did not run (identical planes)"
    else:
        _same_bits(default, walk, (p, "default"))
    _check(default.cpu().numpy(), oe.predict(prm, s["X"]), (p, "gbm"))


@pytest.mark.parametrize("p", [12, 13, 15, 16])
def test_forest_route_boundaries(hip, p, monkeypatch):
    """50 x 70 cells (>= 32 rows: strips and the wave-uniform prefix are on; five by four wave tiles: two blocks, ragged on both
    sides), 9 trees of ~60 nodes with a split on every predictor.  What launch_forest selects, by its conditions:

      p = 12  default and MHS_RF_KERNEL=cbs: rf_walk_cbs_kernel (p <= RF_PREFIX_MAX_P, the loader-wave kernel's keys do not fit);
              db: rf_walk_db_kernel<1>; compact: rf_walk_compact_kernel
      p = 13  cbs no longer applies (the prefix holds 12 predictors): default = db = cbs = rf_walk_db_kernel<1> from the root;
              compact: rf_walk_compact_kernel
      p = 15  as p = 13; the last p of the compact form (p * 16 <= 255: a key's byte offset)
      p = 16  compact does not apply either: MHS_RF_KERNEL=compact falls through to the node walk; default = db =
              rf_walk_db_kernel<1> (p * 8 <= 255 holds up to p = 31)

    Every walk kernel gives the node walk's bits by design, so the forcing variable is the evidence of which one ran; each
    forcing, with and without MHS_RF_PLAIN=1 (no prefix, no early exit), must equal MHS_TREES_GENERIC=1 bit for bit, NA cells
    included, and the oracle to its tolerance."""
    from machisplin_amd import synth
    s = _setup(hip, p - 2, dtype=DTYPES[p % 3], nrow=50, ncol=70)
    prm = synth.rf_params(s["Xs"], s["ys"], 11, n_trees=9)
    bv = prm["best_var"][prm["status"] == -3] - 1
    assert np.isin(np.arange(p), bv).all(), "a predictor without a split"
    m = hip.models.from_param_dict(prm)
    walk = _with_env(monkeypatch, {"MHS_TREES_GENERIC": "1"}, lambda: hip.predict(s["stack"], m))
    win = (3, 47, 5, 66)
    walk_win = _with_env(monkeypatch, {"MHS_TREES_GENERIC": "1"}, lambda: hip.predict(s["stack"], m, window=win))
    for pick in (None, "cbs", "db", "compact", "ld", "sub"):
        for plain in (False, True):
            envs = dict(({"MHS_RF_KERNEL": pick} if pick else {}), **({"MHS_RF_PLAIN": "1"} if plain else {}))
            _same_bits(_with_env(monkeypatch, envs, lambda: hip.predict(s["stack"], m)), walk, (p, envs))
            _same_bits(_with_env(monkeypatch, envs, lambda: hip.predict(s["stack"], m, window=win)), walk_win, (p, envs, win))
    assert s["torch"].isnan(walk).any()
    _check(walk.cpu().numpy(), oe.predict(prm, s["X"]), (p, "rf"))


# ------------------------------------------------------------------------------------------------------ refusals --
def test_loaders_name_the_limit_they_refuse_at(hip):
    """nnet and ksvm are compiled for P <= 12, every loader stops at 64: MhsError at load, the limit in the message, and the
    library goes on."""
    from machisplin_amd import synth
    rng = np.random.default_rng(1)
    X13, X65, y = rng.normal(size=(40, 13)), rng.normal(size=(40, 65)), rng.normal(size=40)
    with pytest.raises(hip.MhsError, match="12 predictors"):
        hip.models.Nnet(rng.normal(size=14 * 10 + 11), 13)
    q = synth.svr_params(X13, y, 1)
    with pytest.raises(hip.MhsError, match="12 predictors"):
        hip.models.from_param_dict(q)
    for prm in (synth.lm_params(X65, y), synth.earth_params(X65, y, 1), synth.gbm_params(X65, y, 1, n_trees=3),
                synth.rf_params(X65, y, 1, n_trees=2)):
        with pytest.raises(hip.MhsError, match="2 .. 64"):
            hip.models.from_param_dict(prm)
    s = _setup(hip, 10)                                    # p = 12 right afterwards
    for k in "nv":
        prm = s["params"][k]
        _check(hip.predict(s["stack"], hip.models.from_param_dict(prm)).cpu().numpy(), oe.predict(prm, s["X"]), k)


# ---------------------------------------------------------------------------- ksvm models at the loops' edges --
def _svr_bundle(hip):
    """One synth.svr_params bundle at p = 5 on float64 planes (450 stations: 270 support vectors, each the scaled predictors of a
    cell of the grid), b set to a value that shows in a far cell, and the planes with a far block: rows 0 .. 2, columns 0 .. 19 of
    layer 0 lifted by 1e7 standard deviations, so that exp(-sigma d^2) is zero for every support vector there."""
    from machisplin_amd import synth
    key = "svr_edges"
    if key not in _CACHE:
        s = _setup(hip, 3, dtype="f64", n=450, seed=7)
        prm = dict(synth.svr_params(s["Xs"], s["ys"], 7))
        prm["b"] = 0.3
        planes = s["stack"].planes.clone()
        far = s["torch"].zeros((9, 190), dtype=s["torch"].bool, device=planes.device)
        far[:3, :20] = True
        planes[0][far] += 1e7 * float(prm["x_scale"][0])
        host = planes.cpu().numpy().astype(np.float64)
        x, y = otps.cell_centres(s["g"].xmin, s["g"].ymax, s["g"].xres, s["g"].yres, 9, 190)
        X = oe.stack_predictors(host, (x, y))
        _CACHE[key] = (s, prm, hip.RasterStack(s["g"], planes, float("nan")), X, far.cpu().numpy().ravel())
    return _CACHE[key]


def _svr_variants(prm):
    a, sv = np.asarray(prm["alpha"]), np.asarray(prm["sv"])
    mixed = np.abs(a) * np.where(np.arange(a.size) % 2 == 0, 1.0, -1.0)
    out = []
    for nsv in (1, 3, 4, 5, 127, 128, 129, 256, 257):                      # the 4-vector unroll and the 128-vector chunk
        out.append(("mixed_%d" % nsv, mixed[:nsv], sv[:nsv]))
    for nsv in (129, 257):
        out.append(("positive_%d" % nsv, np.abs(a[:nsv]), sv[:nsv]))        # npos = nsv: the negative range is empty
        out.append(("negative_%d" % nsv, -np.abs(a[:nsv]), sv[:nsv]))       # npos = 0: the positive range is empty
        out.append(("npos128_%d" % nsv, np.abs(a[:nsv]) * np.where(np.arange(nsv) < 128, 1.0, -1.0), sv[:nsv]))
    tiny = mixed[:131].copy()
    tiny[5] = 1e-12 * np.abs(tiny).max()
    out.append(("tiny_alpha", tiny, sv[:131]))
    out.append(("fitted_270", a, sv))
    return out


@pytest.mark.parametrize("name", [v[0] for v in _svr_variants({"alpha": np.ones(270), "sv": np.zeros((270, 5))})])
def test_ksvm_at_the_edges_of_its_loops(hip, name, monkeypatch):
    """Support-vector counts around the 4-vector unroll and the 128-vector chunk, models whose alphas share one sign (mhs_svr_load
    sorts the positive alphas first: an empty range on one side), npos = 128 exactly, an alpha 1e-12 of the largest -- each
    through svr_rt_kernel (the 9 x 190 grid), svr_kernel (MHS_SVR_NO_ROWTILE=1) and points mode, against the oracle.  The
    plane holds a block of cells beyond the reach of every support vector (every term flushed: y_center - b * y_scale) and, the
    support vectors being cells of this grid, cells that coincide with one."""
    s, base, stack, X, far = _svr_bundle(hip)
    alpha, sv = next((a, v) for n, a, v in _svr_variants(base) if n == name)
    prm = dict(base, alpha=alpha, sv=sv)
    m = hip.models.from_param_dict(prm)
    want = oe.predict(prm, X)
    far = far & ~np.isnan(want)
    assert far.sum() > 50 and (want[far] == prm["y_center"] - prm["b"] * prm["y_scale"]).all() and np.nanstd(want[~far]) > 0
    if sv.shape[0] >= 127:                                                 # some cell's scaled predictors ARE a support vector
        cells = {tuple(z) for z in (X - prm["x_center"]) / prm["x_scale"]}
        assert any(tuple(v) in cells for v in sv)
    rowtile = hip.predict(stack, m).cpu().numpy().ravel()
    plain = _with_env(monkeypatch, {"MHS_SVR_NO_ROWTILE": "1"}, lambda: hip.predict(stack, m)).cpu().numpy().ravel()
    _check(rowtile, want, (name, "svr_rt_kernel"))
    _check(plain, want, (name, "svr_kernel"))
    assert np.nanmax(np.abs(rowtile[far] - want[far])) <= _tol(want) and np.nanmax(np.abs(plain[far] - want[far])) <= _tol(want)
    pts = m.predict_points(s["Xs"])
    ref = oe.predict(prm, s["Xs"])
    assert np.abs(pts - ref).max() <= _tol(ref), name
