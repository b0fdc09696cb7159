"""GPU: Step 1 of machisplin.mltps on the device -- cv.fit_nnet_folds / cv.fit_ksvm_folds (a layer's fold models of a
member in one call) and cv.fit_layer (V73:220-620: fold labels, six members times the folds, hold-out residuals, weight
search, final fits of the kept members), whose result is a ``fitted[i]`` of mltps.mltps.  The fold models are compared
with the single fits on the same rows, the residual columns with the oracle's evaluation of the fitted parameters."""
import numpy as np
import pytest

from oracle import ensemble as oe

pytestmark = pytest.mark.gpu


def _data(n=300, p=5, seed=0):          # the generator of tests/test_learn_fit_gpu.py
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p)) * np.array([1, 2, 3, 1, 5.0, 2, 1])[:p] + np.arange(p)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rng.normal(size=n)
    return rng, X, y


def test_fold_fits_are_the_single_fits_on_the_training_rows(hip):
    cv, models = hip.cv, hip.models
    n, nfolds, p = 600, 10, 5
    rng, X, y = _data(n, p, seed=8)
    kfolds = cv.kfold(n, nfolds, seed=4)
    nn = cv.fit_nnet_folds(X, y, kfolds, seed=6, maxit=50)
    sv = cv.fit_ksvm_folds(X, y, kfolds, sigma=0.2, seed=6)
    assert len(nn) == len(sv) == nfolds
    for v in range(1, nfolds + 1):
        tr = cv.train_rows(kfolds, v, n)
        assert tr.size == n - int(np.sum(kfolds == v))
        assert np.array_equal(nn[v - 1].wts0, np.random.default_rng([6, v - 1]).uniform(-0.7, 0.7, (p + 1) * 10 + 11))
        one = models.Nnet.fit(X[tr], y[tr], nn[v - 1].wts0, maxit=50)
        assert np.array_equal(one.wts, nn[v - 1].wts) and one.value == nn[v - 1].value and one.counts == nn[v - 1].counts
        ksv = models.Ksvm.fit(X[tr], y[tr], 0.2)
        assert np.array_equal(ksv.beta, sv[v - 1].beta) and ksv.params["b"] == sv[v - 1].params["b"] and ksv.n_iter == sv[v - 1].n_iter
    # the hold-out residual columns are resp - (the oracle's evaluation of the fitted parameters), in fold order
    R = cv.cv_residuals([{"n": a, "v": b} for a, b in zip(nn, sv)], X, y, kfolds, "nv")
    want = []
    for v in range(1, nfolds + 1):
        ho, tr = cv.holdout_rows(kfolds, v, n), cv.train_rows(kfolds, v, n)
        mn = y[tr].min()
        prm = oe.nnet_model(nn[v - 1].wts, p, 10, (y[tr] - mn).max(), mn)
        want.append(np.column_stack([y[ho] - oe.predict_nnet(prm, X[ho]), y[ho] - oe.predict(sv[v - 1].params, X[ho])]))
    want = np.concatenate(want)
    assert R.shape == want.shape == (n, 2)
    assert np.abs(R - want).max() < 1e-11 * np.abs(y).max()
    # kernlab's automatic width, fold by fold
    auto = cv.fit_ksvm_folds(X, y, kfolds, seed=6)
    for v in range(1, nfolds + 1):
        tr = cv.train_rows(kfolds, v, n)
        assert auto[v - 1].sigma == float(np.mean(models.sigest(X[tr], seed=[6, v - 1])[[0, 2]]))
        assert auto[v - 1].params["sigma"] == auto[v - 1].sigma


def test_nnet_folds_train_on_the_fold_itself_past_4000_rows(hip):
    cv, models = hip.cv, hip.models
    n, nfolds = 4100, 4
    rng, X, y = _data(n, 5, seed=9)
    kfolds = cv.kfold(n, nfolds, seed=1)
    nn = cv.fit_nnet_folds(X, y, kfolds, seed=2, maxit=10)
    for v in range(1, nfolds + 1):
        tr = np.flatnonzero(kfolds == v)                                      # V73:228-229
        assert np.array_equal(cv.train_rows(kfolds, v, n), tr)
        one = models.Nnet.fit(X[tr], y[tr], nn[v - 1].wts0, maxit=10)
        assert np.array_equal(one.wts, nn[v - 1].wts) and one.counts == nn[v - 1].counts
    R = cv.cv_residuals([{"n": m} for m in nn], X, y, kfolds, "n")
    assert R.shape == (nfolds * n - n, 1)                                     # every row is held out nfolds - 1 times


LAYER = dict(nfolds=3, gbm_fold=dict(n_folds=3, learning_rate=0.05, max_trees=3000),
             gbm_final=dict(n_folds=3, learning_rate=0.05, max_trees=3000), rf=dict(n_trees=15), earth=dict(nfold=0),
             nnet=dict(maxit=200), ksvm=dict(sigma=0.2))


def _layer_data():
    rng = np.random.default_rng(21)                                           # the data of test_gbm_step
    n = 600
    X = rng.normal(size=(n, 5))
    y = 3.0 * np.sin(X[:, 0]) + X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=n)
    return X, y


def test_fit_layer(hip):
    from machisplin_amd import synth
    cv, models = hip.cv, hip.models
    X, y = _layer_data()
    fit = cv.fit_layer(X, y, seed=5, **LAYER)
    assert np.array_equal(fit["kfolds"], cv.kfold(600, 3, 5))
    assert fit["residuals"].shape == (600, 6) and len(fit["fold_models"]) == 3
    assert all(sorted(f) == sorted("bgnmrv") for f in fit["fold_models"])
    p, kept, wts, tot = cv.optx_weights(fit["residuals"])
    assert np.array_equal(p, fit["p"]) and kept == fit["labels"] and wts == fit["weights"] and tot == fit["wt_total"]
    assert len(kept) >= 1 and [m.label for m in fit["models"]] == list(kept)
    assert all(isinstance(m, models.Model) and m.p == 5 for m in fit["models"])
    again = cv.fit_layer(X, y, seed=5, **LAYER)
    assert np.array_equal(again["residuals"], fit["residuals"]) and again["weights"] == fit["weights"]
    assert again["labels"] == fit["labels"] and again["wt_total"] == fit["wt_total"]
    for a, b in zip(again["models"], fit["models"]):
        assert np.array_equal(a.predict_points(X[:40]), b.predict_points(X[:40]))
    # the result is a fitted[i] of mltps(): Steps 2-5 run on it
    g = synth.grid(64, 64)
    planes, nodata = synth.covariates(g, 3, 7, dtype="f32")
    stack = hip.RasterStack(g, planes, nodata)
    xy = synth.stations(g, 600, 7)[0]
    out = hip.mltps_predict(stack, xy, y, fit["models"], fit["weights"], fit["wt_total"])
    assert np.isfinite(out["rsq_model"]) and tuple(out["final"].shape) == (64, 64)


def test_fit_layer_smooth_only_fits_no_tree(hip):
    cv = hip.cv
    X, y = _layer_data()
    fit = cv.fit_layer(X, y, seed=5, smooth_only=True, **LAYER)
    assert fit["residuals"].shape == (600, 4)
    assert all(sorted(f) == sorted("gnmv") for f in fit["fold_models"])
    assert "b" not in fit["labels"] and "r" not in fit["labels"] and set(fit["labels"]) <= set("gnmv")
    p, kept, wts, tot = cv.optx_weights(fit["residuals"], smooth_only=True)
    assert kept == fit["labels"] and wts == fit["weights"] and tot == fit["wt_total"]
    assert [m.label for m in fit["models"]] == list(kept)


def test_fit_layer_final_fits_of_all_six_members(hip, monkeypatch):
    """Every final-fit branch, whatever the weight search keeps on these data: optx_weights is made to keep all six.  The
    finals draw from ``default_rng([seed, member, nfolds])`` (member = place in "bgnmrv"), take the scalar keywords of
    their member's dict, and ``b`` takes the ``gbm_final`` overrides on top of tree_complexity = 5."""
    cv, models = hip.cv, hip.models
    X, y = _layer_data()
    n, seed, nf = 600, 5, 3
    monkeypatch.setattr(cv, "optx_weights", lambda R, smooth_only=False: (np.full(6, 0.5), "bgnmrv", [0.5] * 6, 3.0))
    args = {**LAYER, "earth": dict(nfold=3), "ksvm": dict(), "gbm_final": dict(n_folds=3, learning_rate=0.04, max_trees=3000)}
    fit = cv.fit_layer(X, y, seed=seed, **args)
    assert fit["labels"] == "bgnmrv" and [m.label for m in fit["models"]] == list("bgnmrv") and fit["wt_total"] == 3.0
    b, g, nn, m, r, v = fit["models"]
    # b: machisplin.gbm.step on all rows from the int seed of the stream [seed, 0, nfolds], V73:493's arguments overridden
    s_b = int(np.random.SeedSequence([seed, 0, nf]).generate_state(1)[0])
    assert np.array_equal(b.fold_vector, np.resize(np.arange(1, 4), n)[np.random.default_rng(s_b).permutation(n)])
    assert b._grow["depth"] == 5 and b._grow["shrinkage"] == 0.04 and b._grow["bag_fraction"] == 0.5 and b.n_trees <= 3000
    assert fit["fold_models"][0]["b"]._grow["depth"] == 25 and fit["fold_models"][0]["b"]._grow["shrinkage"] == 0.05
    assert np.array_equal(g.coefficients, models.Gam.fit(X, y).coefficients)
    # n: initial weights from [seed, 2, nfolds], maxit forwarded, the all-rows scaling
    assert np.array_equal(nn.wts0, np.random.default_rng([seed, 2, nf]).uniform(-0.7, 0.7, 71))
    one = models.Nnet.fit(X, y, nn.wts0, maxit=200)
    assert np.array_equal(one.wts, nn.wts) and nn.counts[1] <= 200
    # m: the sub-model folds from [seed, 3, nfolds], nfold forwarded
    assert np.array_equal(m.fold, np.resize(np.arange(1, 4), n)[np.random.default_rng([seed, 3, nf]).permutation(n)])
    assert len(m.cv_models) == 3
    # r: bags, then the per-tree draw seeds, from [seed, 4, nfolds]; n_trees forwarded
    rng = np.random.default_rng([seed, 4, nf])
    bags = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(15)])
    assert r.n_trees == 15 and np.array_equal(r.inbag, bags)
    assert np.array_equal(r.seeds, rng.integers(0, 2 ** 64, size=15, dtype=np.uint64))
    # v: kernlab's automatic width from [seed, 5, nfolds]
    assert v.sigma == float(np.mean(models.sigest(X, seed=[seed, 5, nf])[[0, 2]]))
    # no final shares the fold-label stream default_rng(seed), and the fold models keep theirs: fold 1 of r from [seed, 4, 0]
    rng0 = np.random.default_rng([seed, 4, 0])
    n0 = int(np.sum(fit["kfolds"] != 1))
    assert np.array_equal(fit["fold_models"][0]["r"].inbag[0], np.bincount(rng0.integers(0, n0, size=n0), minlength=n0))
