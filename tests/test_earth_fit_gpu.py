"""GPU: earth (MARS) models fitted on the device (mhs_earth_fit_many through models.Earth.fit / earth_fit_many /
cv.fit_earth_folds) against the numpy restatement of the rule (tests/earth_ref.py).  The yardstick is the certificate
earth_ref.check_model, which follows the device's own choices and recomputes every candidate; on the committed inputs
the reference decides no step inside the tie window (test_earth_ref_host.py), so neither may the device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import earth_inputs as ei
import earth_ref
from oracle import ensemble as oe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("selected", "rss_per_subset", "gcv_per_subset", "prune_terms")


def _record(m):
    rec = {k: getattr(m, k) for k in ARRAYS + ("forward", "rss", "gcv", "rsq", "grsq")}
    rec.update(coef=m.params["coef"], dirs=m.params["dirs"], cuts=m.params["cuts"])
    return rec


def _certify(m, X, y, allowed=0, **kw):
    decided = earth_ref.check_model(X, y, _record(m), **kw)
    print("terms", len(m.params["coef"]), "of", len(m.selected), "stop", m.forward["stop"], "steps decided inside the window", decided)
    assert decided <= allowed
    return decided


def _bit_equal(a, b):
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ARRAYS)
            and all(np.array_equal(a.params[k], b.params[k]) for k in ("coef", "dirs", "cuts"))
            and all(np.array_equal(a.forward[k], b.forward[k]) for k in ("dirs", "cuts", "rss")) and a.forward["stop"] == b.forward["stop"]
            and (a.rss, a.gcv, a.rsq, a.grsq) == (b.rss, b.gcv, b.rsq, b.grsq))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(nk=7), dict(minspan=1, endspan=1)], ids=["default", "nk7", "span1"])
@pytest.mark.parametrize("name", ["small", "stations"])
def test_certificate(hip, name, kw):
    """n = 300 / p = 5 and n = 813 / p = 7: the certificate passes and no step is decided inside the tie window (the
    reference's own count on these inputs is 0)"""
    X, y = ei.COMMITTED[name]()
    m = hip.models.Earth.fit(X, y, **kw)
    _certify(m, X, y, **kw)
    assert len(m.selected) > 3
    if "nk" in kw:
        assert len(m.selected) <= 7 and m.forward["stop"] == "nk"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_edges_wave_boundaries(hip, n):
    """a sorted order that ends at, before and after a wave's 64 rows"""
    X, y = ei.edge(n)
    _certify(hip.models.Earth.fit(X, y), X, y)


@pytest.mark.gpu
def test_edges_variables(hip):
    X, y = ei.two_predictors()
    _certify(hip.models.Earth.fit(X, y), X, y)
    # a 0 / 1 variable has no eligible knot: it enters linearly or not at all
    X, y = ei.binary_variable()
    m = hip.models.Earth.fit(X, y)
    _certify(m, X, y)
    used = m.forward["dirs"][:, 1]
    assert np.any(used != 0) and np.all(used[used != 0] == 2)
    # a constant variable never enters
    X, y = ei.constant_variable()
    m = hip.models.Earth.fit(X, y)
    _certify(m, X, y)
    assert np.all(m.forward["dirs"][:, 2] == 0) and len(m.selected) > 1
    # heavy ties in x: every cut is a data value at a distinct-value boundary
    X, y = ei.heavy_ties()
    m = hip.models.Earth.fit(X, y, minspan=1, endspan=1)
    _certify(m, X, y, minspan=1, endspan=1)
    terms = earth_ref.terms_from(m.forward["dirs"], m.forward["cuts"])
    assert any(d in (1, -1) for _, d, _ in terms)
    for v, d, t in terms:
        if d in (1, -1):
            xs = np.sort(X[:, v])
            j = int(np.searchsorted(xs, t, side="left"))
            assert xs[j] == t and j >= 1 and xs[j - 1] < t


@pytest.mark.gpu
def test_edges_stopping(hip):
    # constant y: intercept only, predictions exactly y
    X, _ = ei.small()
    yc = np.full(300, 2.5)
    m = hip.models.Earth.fit(X, yc)
    _certify(m, X, yc)
    assert m.forward["stop"] == "constant" and len(m.selected) == 1 and np.all(m.predict_points(X) == 2.5)
    # y exactly linear in one variable: one step, then rsq.  The hinges of that variable add nothing to its linear
    # term, so that one step is decided inside the window by construction (the reference's own count here is 1)
    X, y = ei.linear_response()
    m = hip.models.Earth.fit(X, y)
    _certify(m, X, y, allowed=1)
    steps = earth_ref.steps_from(earth_ref.terms_from(m.forward["dirs"], m.forward["cuts"]))
    assert m.forward["stop"] == "rsq" and len(steps) == 1 and steps[0][0] == 1
    assert np.abs(m.predict_points(X) - y).max() <= 1e-12 * np.abs(y).max()
    # nk = 2: intercept only; nk = 3: exactly one pair
    X, y = ei.small()
    m = hip.models.Earth.fit(X, y, nk=2)
    _certify(m, X, y, nk=2)
    assert m.forward["stop"] == "nk" and len(m.selected) == 1
    m = hip.models.Earth.fit(X, y, nk=3)
    _certify(m, X, y, nk=3)
    steps = earth_ref.steps_from(earth_ref.terms_from(m.forward["dirs"], m.forward["cuts"]))
    assert m.forward["stop"] == "nk" and len(m.selected) == 3 and len(steps) == 1 and steps[0][1] == 1


def _coef_error(m, X, y):
    """|B beta_dev - B beta_ref|_inf / max|y|, beta_ref = lstsq on the device's own selected basis"""
    B = earth_ref.basis(X, m.params["dirs"], m.params["cuts"])
    ref = np.linalg.lstsq(B, y, rcond=None)[0]
    return np.abs(B @ m.params["coef"] - B @ ref).max() / np.abs(y).max()


def _reference_coef_error(X, y):
    """the same quantity between the reference's float64 and extended-precision coefficients"""
    a, b = earth_ref.fit(X, y), earth_ref.fit(X, y, acc=np.longdouble)
    assert earth_ref.same_structure(a, b)
    B = earth_ref.basis(X, a["dirs"], a["cuts"])
    return np.abs(B @ a["coef"] - B @ b["coef"]).max() / np.abs(y).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "stations"])
def test_coefficients_and_evaluators(hip, name):
    """|B beta_dev - B beta_ref|_inf / max|y| against 100 x the reference's own float64-versus-longdouble value of the
    same quantity on the same input, ceiling 1e-8.  Measured (reference, CPU): small 1.7e-15, stations 2.7e-15, so the
    bounds are 1.7e-13 and 2.7e-13.  Measured on the device (MI355X): 1.6e-15 and 2.8e-15.  Every figure is printed."""
    X, y = ei.COMMITTED[name]()
    m = hip.models.Earth.fit(X, y)
    ref_err = _reference_coef_error(X, y)
    bound = min(100.0 * ref_err, 1e-8)
    err = _coef_error(m, X, y)
    print(name, "coefficient error: device", err, "reference f64 vs longdouble", ref_err, "bound", bound)
    assert err <= bound
    tol = 1e-12 * np.abs(y).max()
    assert np.abs(m.predict_points(X) - oe.predict(m.params, X)).max() <= tol
    # the loaders' path: the dict round-trips
    again = hip.models.from_param_dict(m.params)
    assert np.array_equal(again.predict_points(X), m.predict_points(X))


@pytest.mark.gpu
def test_beyond_the_on_chip_rows(hip):
    """n just above EARTH_LDS_ROWS: the residual and the working column are read from device memory by the same code"""
    src = open(os.path.join(ROOT, "machisplin_amd", "csrc", "earth_fit.hip")).read()
    limit = int(re.search(r"constexpr int EARTH_LDS_ROWS = (\d+);", src).group(1))
    X, y = ei.large(limit + 104)
    assert limit == 4096 and limit < y.size <= limit + 1024
    m = hip.models.Earth.fit(X, y)
    _certify(m, X, y)
    assert np.abs(m.predict_points(X) - oe.predict_earth(m.params, X)).max() <= 1e-12 * np.abs(y).max()
    print("coefficient error: device", _coef_error(m, X, y))


@pytest.mark.gpu
def test_reproducible_and_batch_independent(hip):
    X, y = ei.stations()
    a = hip.models.Earth.fit(X, y)
    b = hip.models.Earth.fit(X, y)
    assert _bit_equal(a, b)
    Xs, ys = ei.small()
    Xl, yl = ei.shape(1500, 5, 21)
    batch = hip.models.earth_fit_many([Xl, X[:, :5], Xs], [yl, y, ys])
    alone = hip.models.Earth.fit(X[:, :5], y)
    assert _bit_equal(batch[1], alone)
    assert _bit_equal(batch[2], hip.models.Earth.fit(Xs, ys)) and _bit_equal(batch[0], hip.models.Earth.fit(Xl, yl))


@pytest.mark.gpu
def test_nfold(hip):
    """Earth.fit(nfold = 10, fold = given): every cv_rsq_folds[f] is the value recomputed from a separate fit on fold != f"""
    X, y, fold = ei.folds()
    m = hip.models.Earth.fit(X, y, nfold=10, fold=fold)
    assert _bit_equal(m, hip.models.Earth.fit(X, y)) and len(m.cv_models) == 10 and m.cv_rsq_folds.shape == (10,)
    for f in range(1, 11):
        tr, ho = np.flatnonzero(fold != f), np.flatnonzero(fold == f)
        sub = hip.models.Earth.fit(X[tr], y[tr])
        assert _bit_equal(sub, m.cv_models[f - 1])
        d = y[ho] - oe.predict(sub.params, X[ho])
        want = 1.0 - float(d @ d) / float(((y[ho] - y[ho].mean()) ** 2).sum())
        assert abs(m.cv_rsq_folds[f - 1] - want) <= 1e-10
    assert m.cv_rsq == pytest.approx(np.mean(m.cv_rsq_folds), abs=1e-15) and 0.5 < m.cv_rsq < 1.0
    # drawn folds: a permutation of rep(1 .. nfold), the same for the same seed
    c = hip.models.Earth.fit(X, y, nfold=5, seed=3)
    d = hip.models.Earth.fit(X, y, nfold=5, seed=3)
    e = hip.models.Earth.fit(X, y, nfold=5, seed=4)
    assert np.array_equal(c.fold, d.fold) and not np.array_equal(c.fold, e.fold) and np.array_equal(np.bincount(c.fold)[1:], [120] * 5)
    assert np.array_equal(c.cv_rsq_folds, d.cv_rsq_folds)


@pytest.mark.gpu
def test_fit_earth_folds(hip):
    """10 folds of n = 600 in one call: every fold model is Earth.fit on its training rows, and the m column of
    cv_residuals is resp - the oracle's prediction"""
    X, y, kfolds = ei.folds()
    models = hip.cv.fit_earth_folds(X, y, kfolds, nfold=10, seed=3)
    assert len(models) == 10 and all(len(m.cv_models) == 10 for m in models)
    want = []
    for v, m in enumerate(models, start=1):
        tr = hip.cv.train_rows(kfolds, v, 600)
        assert _bit_equal(m, hip.models.Earth.fit(X[tr], y[tr]))
        ho = hip.cv.holdout_rows(kfolds, v, 600)
        want.append(y[ho] - oe.predict(m.params, X[ho]))
    got = hip.cv.cv_residuals([{"m": m} for m in models], X, y, kfolds, labels="m")
    assert got.shape == (600, 1)
    assert np.abs(got[:, 0] - np.concatenate(want)).max() <= 1e-12 * np.abs(y).max()
    tr = hip.cv.train_rows(kfolds, 4, 600)
    _certify(models[3], X[tr], y[tr])
    plain = hip.cv.fit_earth_folds(X, y, kfolds, nfold=0)
    assert all(_bit_equal(a, b) and not hasattr(a, "cv_rsq") for a, b in zip(plain, models))


@pytest.mark.gpu
def test_errors(hip):
    import ctypes as C
    from machisplin_amd import _lib
    X, y = ei.small()

    def refused(X=X, y=y, **kw):
        with pytest.raises(hip.MhsError) as e:
            hip.models.Earth.fit(X, y, **kw)
        assert e.value.code == _lib.ERR_INVALID

    Xn = X.copy()
    Xn[17, 2] = np.nan
    refused(X=Xn)
    Xi = X.copy()
    Xi[3, 0] = np.inf
    refused(X=Xi)
    yi = y.copy()
    yi[5] = np.inf
    refused(y=yi)
    yn = y.copy()
    yn[6] = np.nan
    refused(y=yn)
    refused(X=X[:1], y=y[:1])                        # n < 2
    refused(X=X[:, :1])                              # p below mhs_earth_load's range
    refused(X=np.zeros((10, 65)), y=np.zeros(10), nk=5)          # p above it
    refused(nk=66)                                   # above MHS_EARTH_MAX_NK
    refused(X=np.random.default_rng(0).uniform(size=(100, 40)), y=y[:100])      # p > 32: the default nk is 81
    refused(thresh=-1e-3)
    refused(penalty=-1.0)
    h = (C.c_void_p * 1)()
    ns = np.array([300], dtype=np.int64)
    assert _lib.lib().mhs_earth_fit_many(1, None, None, ns.ctypes.data, 5, 0, 0.001, 2.0, 0, 0, h) == _lib.ERR_INVALID
    Xf = np.asfortranarray(X)
    pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    assert _lib.lib().mhs_earth_fit_many(1, pa(Xf), pa(y), ns.ctypes.data, 5, 0, 0.001, 2.0, 0, 0, None) == _lib.ERR_INVALID
    # p = 40 with an explicit nk is accepted
    Xw = np.round(np.random.default_rng(1).uniform(size=(120, 40)), 3)
    assert len(hip.models.Earth.fit(Xw, y[:120], nk=9).selected) <= 9
    # mhs_earth_get is for fitted models only
    m = hip.models.Earth.fit(X, y)
    loaded = hip.models.from_param_dict(m.params)
    a, b = C.c_int(), C.c_int()
    none = [None] * 12
    assert _lib.lib().mhs_earth_get(loaded._h, C.byref(a), C.byref(b), *none) == _lib.ERR_INVALID
    assert _lib.lib().mhs_earth_get(m._h, C.byref(a), C.byref(b), *none) == _lib.OK and (a.value, b.value) == (len(m.params["coef"]), len(m.selected))
    gam = hip.models.Gam.fit(X, y)
    assert _lib.lib().mhs_earth_get(gam._h, C.byref(a), C.byref(b), *none) == _lib.ERR_INVALID


_BEFORE_INIT = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from machisplin_amd import _lib
lib = _lib.load()
n, p = 50, 3
X = np.asfortranarray(np.random.default_rng(0).normal(size=(n, p))); y = X[:, 0].copy()
pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
ns = np.array([n], dtype=np.int64); h = (C.c_void_p * 1)()
rc = lib.mhs_earth_fit_many(1, pa(X), pa(y), ns.ctypes.data, p, 0, 0.001, 2.0, 0, 0, h)
sys.exit(0 if rc == _lib.ERR_NODEVICE else 1)
"""


def test_call_before_init_is_refused():
    """a fresh process that has not called mhs_init: MHS_ERR_NODEVICE (with or without a GPU in the machine)"""
    assert subprocess.run([sys.executable, "-c", _BEFORE_INIT, ROOT], timeout=300).returncode == 0
