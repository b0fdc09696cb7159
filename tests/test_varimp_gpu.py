"""GPU: the variable importance of the other members -- gbm's error reduction out of the growth kernel
(mhs_gbm_grow_many_reduction: Gbm.error_reduction / relative_influence / contributions), the ksvm break-down driven
through predict_points (varimp.ksvm_contributions) -- and cv.fit_layer(var_imp = True), the layer's $var.imp."""
import ctypes as C
import inspect

import numpy as np
import pytest

import gbm_inputs as gi
import gbm_ref
import varimp_ref

pytestmark = pytest.mark.gpu

NODE_KEYS = ("tree_offsets", "split_var", "split_val", "left", "right", "missing")


def _grow_without_reduction(X, y, bags, depth=25, minobs=10, shrinkage=0.01):
    """mhs_gbm_grow_many itself, first call, one model: (F, init_f, the six node arrays)"""
    from machisplin_amd import _lib
    Xf, y = np.asfortranarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    n, p = Xf.shape
    bags = np.ascontiguousarray(bags, dtype=np.int32)
    T, cap = bags.shape[0], bags.shape[0] * (3 * depth + 1)
    F, init, off = np.empty(n), np.zeros(1), np.zeros(T + 1, dtype=np.int64)
    iv = [np.zeros(cap, dtype=np.int32) for _ in range(4)]
    val = np.zeros(cap)
    pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    ns, bs = np.array([n], dtype=np.int64), np.array([bags.shape[1]], dtype=np.int64)
    _lib.check(_lib.lib().mhs_gbm_grow_many(1, pa(Xf), pa(y), ns.ctypes.data, p, pa(bags), bs.ctypes.data, T, depth, minobs, shrinkage, 1,
                                            pa(F), init.ctypes.data, pa(off), pa(iv[0]), pa(val), pa(iv[1]), pa(iv[2]), pa(iv[3])))
    nn = int(off[-1])
    return F, float(init[0]), {"tree_offsets": off, "split_var": iv[0][:nn], "split_val": val[:nn], "left": iv[1][:nn], "right": iv[2][:nn],
                               "missing": iv[3][:nn]}


def test_gbm_error_reduction(hip):
    """gi.short(): the input on which test_exact_against_the_reference finds every device tree identical to gbm_ref's.
    The improvements agree to the relative tolerance that test_gbm_fit_gpu.py grants improvements: gbm_ref.near_tie's rel."""
    rel_tol = inspect.signature(gbm_ref.near_tie).parameters["rel"].default
    X, y, bags = gi.short()
    m = hip.models.Gbm.fit(X, y, 40, bags=bags)
    ref, _, rtrees = gbm_ref.fit(X, y, 40, bags)
    assert all(gbm_ref.same_structure(gbm_ref.tree_of(m.params, t), rtrees[t]) for t in range(40))
    want = np.concatenate([t["imp"] for t in rtrees])
    red = m.error_reduction
    split = m.params["split_var"] >= 0
    assert red.shape == want.shape == split.shape
    rel = np.abs(red - want)[split] / np.maximum(np.abs(red), np.abs(want))[split]
    print("split nodes", int(split.sum()), "max relative difference of the improvements", rel.max())
    assert np.all(red[~split] == 0.0) and np.all(want[~split] == 0.0) and np.all(red[split] > 0.0)
    assert rel.max() <= rel_tol
    # the new entry grows the same trees as mhs_gbm_grow_many, bit for bit
    F, init_f, old = _grow_without_reduction(X, y, bags)
    assert all(np.array_equal(old[k], m.params[k]) for k in NODE_KEYS) and init_f == m.init_f and np.array_equal(F, m.fit)
    # relative.influence: per variable, over the first n_trees trees, in tree and then node order
    for n_trees in (None, 40, 7, 0):
        end = int(m.params["tree_offsets"][40 if n_trees is None else n_trees])
        ri = np.zeros(5)
        for e in range(end):
            if m.params["split_var"][e] >= 0:
                ri[m.params["split_var"][e]] = ri[m.params["split_var"][e]] + red[e]
        assert np.array_equal(m.relative_influence(n_trees), ri)
    # summary.gbm: percent, and the descending order
    rel_inf, order = m.contributions()
    assert abs(rel_inf.sum() - 100.0) <= 1e-12 and np.all(np.diff(rel_inf[order]) <= 0) and sorted(order) == list(range(5))
    assert np.allclose(rel_inf, 100.0 * m.relative_influence() / m.relative_influence().sum(), rtol=1e-15, atol=0)
    assert order[0] == 0                                        # y = sin(x0) + 0.3 x1 + noise
    # gbm.more concatenates
    half = hip.models.Gbm.fit(X, y, 25, bags=bags[:25]).more(15, bags=bags[25:])
    assert np.array_equal(half.error_reduction, red) and np.array_equal(half.relative_influence(), m.relative_influence())
    # a model without a split
    mc = hip.models.Gbm.fit(X, np.full(300, 2.5), 3, bags=bags[:3])
    assert not mc.error_reduction.any() and not mc.contributions()[0].any()


def test_gbm_step_models_carry_it(hip):
    rng = np.random.default_rng(21)
    X = rng.normal(size=(300, 4))
    y = 3.0 * np.sin(X[:, 0]) + X[:, 1] + 0.3 * rng.normal(size=300)
    final = hip.cv.gbm_step(X, y, seed=3, learning_rate=0.05, n_folds=3, max_trees=400)[0]
    for m in [final] + list(final.fold_models):
        assert m.error_reduction.shape == m.params["split_var"].shape
        assert np.array_equal(m.error_reduction > 0, m.params["split_var"] >= 0)
    assert final.contributions()[1][0] == 0


def test_ksvm_contributions(hip):
    from machisplin_amd import varimp
    rng = np.random.default_rng(40)
    X = rng.normal(size=(60, 3)) * np.array([1.0, 2.0, 0.5])
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.05 * rng.normal(size=60)
    m = hip.models.Ksvm.fit(X, y, 0.3)
    f = m.predict_points(X)
    scale = np.abs(f).max()
    C_, b0 = varimp.breakdown_up_many(m.predict_points, X, X)
    worst = 0.0
    for x, c in zip(X, C_):
        c_ref, b_ref = varimp_ref.breakdown_up(m.predict_points, x, X)
        worst = max(worst, np.abs(c - c_ref).max(), abs(b0 - b_ref))
    # sum_v c_v telescopes to (the mean of 60 copies of f(x*)) - b0: a mean of s equal values errs by s 2^-53 of it, the p
    # differences and their sum by another 3 p 2^-53 max|f|
    total = np.abs(C_.sum(axis=1) - (f - b0)).max()
    print("max |c - restatement|", worst, "max |sum c - (f(x*) - b0)|", total, "max|f|", scale)
    assert worst <= 1e-12 * scale
    assert total <= (60 + 3 * 3) * 2.0 ** -53 * scale
    got = varimp.ksvm_contributions(m, X)
    assert got.shape == (3,) and np.array_equal(got, np.mean(np.abs(C_), axis=0)) and got[0] > got[2] > 0
    # more rows than the sample: the sample's rows from their own stream
    rows = np.random.default_rng(9).choice(60, 20, replace=False)
    assert np.array_equal(varimp.ksvm_contributions(m, X, sample=20, seed=9), varimp.ksvm_contributions(m, X, rows=rows))


LAYER = dict(nfolds=3, gbm_fold=dict(n_folds=3, learning_rate=0.05, max_trees=3000),          # the shape of test_step1_gpu.py
             gbm_final=dict(n_folds=3, learning_rate=0.05, max_trees=3000), rf=dict(n_trees=15), earth=dict(nfold=0),
             nnet=dict(maxit=200), ksvm=dict(sigma=0.2))


def test_fit_layer_var_imp(hip, monkeypatch):
    """var_imp = True adds one entry per kept label, each of length p, and changes nothing else -- first with the real
    weight search, whatever it keeps, then with the search made to keep all six members so that every branch runs"""
    from machisplin_amd import synth, varimp
    cv = hip.cv
    rng = np.random.default_rng(21)
    n, p, seed = 600, 5, 5
    X = rng.normal(size=(n, p))
    y = 3.0 * np.sin(X[:, 0]) + X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=n)

    def same_but_for_var_imp(fit, plain):
        assert "var_imp" not in plain and sorted(fit["var_imp"]) == sorted(fit["labels"])
        assert all(len(e) == p and np.all(np.isfinite(e)) for e in fit["var_imp"].values())
        assert np.array_equal(fit["kfolds"], plain["kfolds"]) and np.array_equal(fit["residuals"], plain["residuals"])
        assert np.array_equal(fit["p"], plain["p"]) and fit["labels"] == plain["labels"] and fit["weights"] == plain["weights"]
        assert fit["wt_total"] == plain["wt_total"] and len(fit["models"]) == len(plain["models"]) == len(fit["labels"])
        for a, b in zip(fit["models"], plain["models"]):
            assert a.label == b.label and np.array_equal(a.predict_points(X), b.predict_points(X))

    plain = cv.fit_layer(X, y, seed=seed, **LAYER)
    same_but_for_var_imp(cv.fit_layer(X, y, seed=seed, var_imp=True, **LAYER), plain)
    monkeypatch.setattr(cv, "optx_weights", lambda R, smooth_only=False: (np.full(6, 0.5), "bgnmrv", [0.5] * 6, 3.0))
    fit = cv.fit_layer(X, y, seed=seed, var_imp=True, **LAYER)
    assert fit["labels"] == "bgnmrv" and np.array_equal(fit["residuals"], plain["residuals"])
    for a in fit["models"]:           # a member the real search kept has the same final fit
        if a.label in plain["labels"]:
            assert np.array_equal(a.predict_points(X), plain["models"][plain["labels"].index(a.label)].predict_points(X))
    b, g, nn, m, r, v = fit["models"]
    vi = fit["var_imp"]
    assert np.array_equal(vi["b"], b.contributions()[0]) and abs(vi["b"].sum() - 100.0) <= 1e-12
    assert np.array_equal(vi["g"], g.coefficients[1:])
    assert np.array_equal(vi["n"], varimp.garson(nn.wts, p, 10)) and abs(vi["n"].sum() - 1.0) <= 1e-14
    assert vi["m"].shape == (p, 3) and vi["m"][:, 1].max() == 100.0
    # the forest's permutation seeds and the ksvm sample come from streams of their own
    assert np.array_equal(r.perm_seeds, np.random.default_rng([seed, 4, 3, 1]).integers(0, 2 ** 64, size=15, dtype=np.uint64))
    assert vi["r"].shape == (p, 2) and np.array_equal(vi["r"], r.importance) and np.array_equal(vi["r"][:, 1], r.inc_node_purity)
    rows = np.random.default_rng([seed, 5, 3, 1]).choice(n, 200, replace=False)
    assert np.array_equal(vi["v"], varimp.ksvm_contributions(v, X, rows=rows))
    # the sine term and the interaction outweigh the two idle predictors in every member that can see them
    for lab in "brv":
        col = vi[lab][:, 0] if lab == "r" else vi[lab]
        assert col[:3].min() > col[3:].max(), (lab, col)
    # mltps() hands the entry on with the layer's result
    g64 = synth.grid(64, 64)
    planes, nodata = synth.covariates(g64, 3, 7, dtype="f32")
    stack = hip.RasterStack(g64, planes, nodata)
    xy = synth.stations(g64, n, 7)[0]
    omega = hip.mltps_layers(stack, np.column_stack([xy, y]), [fit])
    assert omega[0]["var_imp"] is fit["var_imp"] and omega[0]["n_layers"] == 1
