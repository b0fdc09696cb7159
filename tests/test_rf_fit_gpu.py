"""GPU: randomForest regression forests grown on the device (mhs_rf_fit_many through models.RandomForest.fit /
rf_fit_many / cv.fit_forest_folds) against the numpy restatement of the growth rule (tests/rf_ref.py).  The yardstick
is the certificate walk rf_ref.check_tree, not tree-versus-tree equality: with nodesize 5 the reference's own float64 and
extended-precision trees already differ in structure (test_rf_ref_host.py, rf_ref's docstring)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rf_inputs as ri
import rf_ref
from oracle import ensemble as oe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tree_offsets",) + rf_ref.KEYS


def _certify(m, X, y, inbag, seeds, mtry, nodesize):
    """every tree of the forest through check_tree; returns the per-tree results"""
    res = [rf_ref.check_tree(X, y, inbag[t], seeds[t], mtry, nodesize, rf_ref.tree_of(m.params, t)) for t in range(inbag.shape[0])]
    ties, internal = sum(r["near_ties"] for r in res), sum(r["internal"] for r in res)
    print("nodes", sum(r["nodes"] for r in res), "internal", internal, "decided by a near-tie", ties,
          "(%.1f %%)" % (100.0 * ties / max(internal, 1)))
    return res


def _bit_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in KEYS)


CASES = [("small", mtry, ns) for mtry in (1, 5) for ns in (1, 5, 40)] + [("stations", mtry, ns) for mtry in (1, 2, 7) for ns in (1, 5, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mtry,nodesize", CASES)
def test_certificate(hip, name, mtry, nodesize):
    """20 trees at n = 300 / p = 5 and n = 813 / p = 7 (rounded: ties in x), mtry in {1, floor(p / 3), p}, nodesize in
    {1, 5, 40}: every tree passes the certificate walk"""
    X, y, inbag, seeds = getattr(ri, name)()
    m = hip.models.RandomForest.fit(X, y, 20, mtry=mtry, nodesize=nodesize, inbag=inbag, seeds=seeds)
    _certify(m, X, y, inbag, seeds, mtry, nodesize)


@pytest.mark.gpu
def test_certificate_edges(hip):
    # segments that end at, just before and just after a wave's 64 rows; every row once
    for n in (63, 64, 65, 129):
        X, y = ri.plain(n, 3, 40 + n)
        inbag = np.ones((4, n), dtype=np.int32)
        seeds = np.arange(4, dtype=np.uint64) + 99
        m = hip.models.RandomForest.fit(X, y, 4, mtry=2, nodesize=1, inbag=inbag, seeds=seeds)
        res = _certify(m, X, y, inbag, seeds, 2, 1)
        assert all(r["nodes"] == 2 * n - 1 for r in res)            # continuous x and y, nodesize 1: one row per leaf
    # nodesize above the population: the root is always tried (only NON-root nodes stop at nodesize), its children stop
    X, y = ri.plain(12, 3, 41)
    inbag, seeds = ri.bags_for(12, 5, 42)
    m = hip.models.RandomForest.fit(X, y, 5, mtry=1, nodesize=40, inbag=inbag, seeds=seeds)
    res = _certify(m, X, y, inbag, seeds, 1, 40)
    assert all(r["nodes"] <= 3 for r in res)
    # constant response: no candidate has a criterion > 0, root-only trees that predict y exactly
    X, _, inbag, seeds = ri.small(5)
    yc = np.full(300, 2.5)
    m = hip.models.RandomForest.fit(X, yc, 5, inbag=inbag, seeds=seeds)
    _certify(m, X, yc, inbag, seeds, 1, 5)
    assert np.array_equal(m.params["tree_offsets"], np.arange(6)) and np.all(m.params["status"] == -1)
    assert np.all(m.params["node_pred"] == 2.5)
    assert np.all(m.predict_points(X) == 2.5)
    # a tree whose bag is one row repeated (between two ordinary trees)
    X, y, inbag, seeds = ri.small(3)
    inbag = inbag.copy()
    inbag[1] = 0
    inbag[1, 17] = 300
    m = hip.models.RandomForest.fit(X, y, 3, mtry=2, inbag=inbag, seeds=seeds)
    res = _certify(m, X, y, inbag, seeds, 2, 5)
    assert res[1]["nodes"] == 1 and res[0]["nodes"] > 1 and res[2]["nodes"] > 1


@pytest.mark.gpu
def test_beyond_the_on_chip_rows(hip):
    """n = 9 000 > RF_LDS_ROWS: y, the counts and the marks are read from device memory by the same code"""
    src = open(os.path.join(ROOT, "machisplin_amd", "csrc", "rf_fit.hip")).read()
    limit = int(re.search(r"constexpr int RF_LDS_ROWS = (\d+);", src).group(1))
    X, y, inbag, seeds = ri.large()
    assert limit == 8192 and limit < y.size <= limit + 1024
    m = hip.models.RandomForest.fit(X, y, inbag.shape[0], inbag=inbag, seeds=seeds)
    _certify(m, X, y, inbag, seeds, 1, 5)
    assert np.abs(m.predict_points(X) - oe.predict(m.params, X)).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.gpu
def test_consistent_with_the_evaluators(hip):
    X, y, inbag, seeds = ri.stations()
    m = hip.models.RandomForest.fit(X, y, 20, inbag=inbag, seeds=seeds)
    assert m.mtry == 2 and m.nodesize == 5
    tol = 1e-12 * np.abs(y).max()
    assert np.abs(m.predict_points(X) - oe.predict(m.params, X)).max() <= tol
    res = _certify(m, X, y, inbag, seeds, 2, 5)
    trees = [rf_ref.tree_of(m.params, t) for t in range(20)]
    for t, (tr, r) in enumerate(zip(trees, res)):
        rows = np.flatnonzero(inbag[t] > 0)
        assert np.array_equal(rf_ref.terminal_nodes(tr, X[rows]), r["leaf"][rows])
    # out-of-bag: the tree-order mean from the device's own trees
    want, cnt = rf_ref.oob(trees, X, inbag)
    assert np.array_equal(m.oob_count, cnt) and cnt.min() >= 0
    seen = cnt > 0
    assert seen.sum() > 800 and np.abs(m.oob_pred[seen] - want[seen]).max() <= tol and np.all(np.isnan(m.oob_pred[~seen]))
    mse = float(np.mean((y[seen] - want[seen]) ** 2))
    rsq = 1.0 - mse / float(np.mean((y[seen] - y[seen].mean()) ** 2))
    assert np.isclose(m.mse, mse, rtol=1e-10, atol=0) and np.isclose(m.rsq, rsq, rtol=1e-10, atol=0)
    # IncNodePurity: the reference's criterion of every split, summed per variable, / n_trees.  A criterion is a
    # difference of sums of squares: its absolute rounding error is a few ulp of the node's sum(c y^2); the nodes of a
    # level partition the bag, a tree has a few dozen levels => well below 1e-12 sum(c y^2) per tree.
    pur = np.zeros(7)
    for tr, r in zip(trees, res):
        internal = tr["status"] == -3
        np.add.at(pur, tr["best_var"][internal] - 1, r["crit"][internal])
    bound = 1e-12 * float(np.mean([(inbag[t] * y * y).sum() for t in range(20)]))
    print("IncNodePurity", m.inc_node_purity, "max diff", np.abs(m.inc_node_purity - pur / 20).max(), "bound", bound)
    assert np.abs(m.inc_node_purity - pur / 20).max() <= bound


@pytest.mark.gpu
def test_reproducible(hip):
    X, y, inbag, seeds = ri.stations()
    a = hip.models.RandomForest.fit(X, y, 20, inbag=inbag, seeds=seeds)
    b = hip.models.RandomForest.fit(X, y, 20, inbag=inbag, seeds=seeds)
    assert _bit_equal(a.params, b.params)
    assert np.array_equal(a.oob_pred, b.oob_pred, equal_nan=True) and np.array_equal(a.inc_node_purity, b.inc_node_purity)
    # alone, and in a batch of three models of different n
    Xs, ys, bs, ss = ri.small()
    Xl, yl = ri.plain(1500, 7, 50)
    bl, sl = ri.bags_for(1500, 20, 51)
    batch = hip.models.rf_fit_many([Xl, X, np.column_stack([Xs, Xs[:, :2]])], [yl, y, ys], 20, inbag=[bl, inbag, bs], seeds=[sl, seeds, ss])
    assert _bit_equal(batch[1].params, a.params)
    assert np.array_equal(batch[1].oob_pred, a.oob_pred, equal_nan=True) and np.array_equal(batch[1].inc_node_purity, a.inc_node_purity)
    # tree t of the 20-tree call is the 1-tree call with its bag and seed
    for t in (0, 7, 19):
        one = hip.models.RandomForest.fit(X, y, 1, inbag=inbag[t:t + 1], seeds=seeds[t:t + 1])
        tr = rf_ref.tree_of(a.params, t)
        assert all(np.array_equal(tr[k], one.params[k]) for k in rf_ref.KEYS)
    # seeded bags and draws
    c = hip.models.RandomForest.fit(Xs, ys, 10, seed=5)
    d = hip.models.RandomForest.fit(Xs, ys, 10, seed=5)
    e = hip.models.RandomForest.fit(Xs, ys, 10, seed=6)
    assert _bit_equal(c.params, d.params) and np.array_equal(c.inbag, d.inbag) and not np.array_equal(c.inbag, e.inbag)
    assert np.all(c.inbag.sum(axis=1) == 300)
    _certify(c, Xs, ys, c.inbag, c.seeds, 1, 5)


@pytest.mark.gpu
def test_fit_forest_folds(hip):
    """10 folds of n = 600 in one call: every fold model is RandomForest.fit on its training rows with the same bags and
    seeds, and the r column of cv_residuals is resp - the oracle's prediction"""
    X, y, kfolds = ri.folds()
    models = hip.cv.fit_forest_folds(X, y, kfolds, n_trees=15, seed=3)
    assert len(models) == 10
    want = []
    for v, m in enumerate(models, start=1):
        tr = hip.cv.train_rows(kfolds, v, 600)
        assert m.inbag.shape == (15, tr.size)
        alone = hip.models.RandomForest.fit(X[tr], y[tr], 15, inbag=m.inbag, seeds=m.seeds)
        assert _bit_equal(alone.params, m.params)
        ho = hip.cv.holdout_rows(kfolds, v, 600)
        want.append(y[ho] - oe.predict(m.params, X[ho]))
    got = hip.cv.cv_residuals([{"r": m} for m in models], X, y, kfolds, labels="r")
    assert got.shape == (600, 1)
    assert np.abs(got[:, 0] - np.concatenate(want)).max() <= 1e-12 * np.abs(y).max()
    rf_ref.check_tree(X[hip.cv.train_rows(kfolds, 4, 600)], y[hip.cv.train_rows(kfolds, 4, 600)], models[3].inbag[2], models[3].seeds[2], 1, 5,
                      rf_ref.tree_of(models[3].params, 2))


@pytest.mark.gpu
def test_quality_sanity(hip):
    """n = 813, 100 trees, default mtry: the OOB R^2 is within 0.05 of scikit-learn's forest of the same shape (loose:
    the bags and the draws differ)"""
    from sklearn.ensemble import RandomForestRegressor
    X, y, _, _ = ri.stations(1)
    m = hip.models.RandomForest.fit(X, y, 100, seed=11)
    sk = RandomForestRegressor(n_estimators=100, max_features=m.mtry, min_samples_split=6, oob_score=True, random_state=0).fit(X, y)
    print("OOB rsq: device", m.rsq, "scikit-learn", sk.oob_score_)
    assert abs(m.rsq - sk.oob_score_) <= 0.05


@pytest.mark.gpu
def test_errors(hip):
    import ctypes as C
    from machisplin_amd import _lib
    X, y, inbag, seeds = ri.small(3)

    def refused(**kw):
        a = dict(X=X, y=y, n_trees=3, inbag=inbag, seeds=seeds)
        a.update(kw)
        with pytest.raises(hip.MhsError) as ei:
            hip.models.RandomForest.fit(a.pop("X"), a.pop("y"), a.pop("n_trees"), **a)
        assert ei.value.code == _lib.ERR_INVALID

    Xn = X.copy()
    Xn[17, 2] = np.nan
    refused(X=Xn)
    yi = y.copy()
    yi[5] = np.inf
    refused(y=yi)
    neg = inbag.copy()
    neg[1, 5] = -1
    refused(inbag=neg)
    zero = inbag.copy()
    zero[2] = 0
    refused(inbag=zero)
    refused(mtry=0)
    refused(mtry=6)
    refused(nodesize=0)
    refused(X=X[:, :1])                              # p below mhs_rf_load's range
    h = (C.c_void_p * 1)()
    ns = np.array([300], dtype=np.int64)
    rc = _lib.lib().mhs_rf_fit_many(1, None, None, ns.ctypes.data, 5, 3, 1, 5, None, None, h, None, None, None)
    assert rc == _lib.ERR_INVALID
    # mhs_rf_get is for fitted forests only
    m = hip.models.RandomForest.fit(X, y, 3, inbag=inbag, seeds=seeds)
    loaded = hip.models.from_param_dict(m.params)
    nn = C.c_int64()
    assert _lib.lib().mhs_rf_get(loaded._h, C.byref(nn), None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert np.array_equal(loaded.predict_points(X), m.predict_points(X))


_BEFORE_INIT = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from machisplin_amd import _lib
lib = _lib.load()
n, p, T = 50, 3, 2
X = np.asfortranarray(np.random.default_rng(0).normal(size=(n, p))); y = X[:, 0].copy()
inbag = np.ones((T, n), dtype=np.int32); seeds = np.arange(T, dtype=np.uint64)
pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
ns = np.array([n], dtype=np.int64); h = (C.c_void_p * 1)()
rc = lib.mhs_rf_fit_many(1, pa(X), pa(y), ns.ctypes.data, p, T, 1, 5, pa(inbag), pa(seeds), h, None, None, None)
sys.exit(0 if rc == _lib.ERR_NODEVICE else 1)
"""


def test_call_before_init_is_refused():
    """a fresh process that has not called mhs_init: MHS_ERR_NODEVICE (with or without a GPU in the machine)"""
    assert subprocess.run([sys.executable, "-c", _BEFORE_INIT, ROOT], timeout=300).returncode == 0
