"""Step 1's data-parallel part: hold-out predictions of the six learners for the
k-fold cross-validation (V73:225-319) on the GPU, and the ensemble weight search that consumes them
(V73:326-393); rank 4: the tree-count search of machisplin.gbm.step over grown fold models (gbm_step_search).

All six members have device fits (models.py; :func:`fit_forest_folds`, :func:`fit_earth_folds`, :func:`fit_nnet_folds`
and :func:`fit_ksvm_folds` fit all fold models of their member in one device call each), :func:`gbm_step` runs
machisplin.gbm.step whole, :func:`kfold` draws the fold labels and :func:`fit_layer` performs Step 1 and the final
fits of one layer (V73:220-620): its result is a ``fitted[i]`` of :func:`mltps.mltps`.  What else runs here is what R does with
``terra::predict(model, test)`` inside the fold loop: every fold's models evaluated at that fold's hold-out
rows through ``mhs_predict_points``, the residual vectors concatenated in fold order, and
``optimx(par = 0.5, lower = 0, upper = 1, method = "L-BFGS-B")`` on

    fit(k) = sum_i ( sum_m k_m r_{i,m} / sum_m k_m )^2 = k' (R'R) k / (1'k)^2 .

The objective is scale-invariant, so the optimiser's end point on the minimising ray decides the rounded
weights (V73:340-362); this module uses SciPy's L-BFGS-B (the same Nocedal/Zhu code base R's optim wraps)
with the same start, bounds and objective -- the iterate sequence of R's build is NOT reproduced bit for
bit, and R-side integration keeps optimx in R."""
from __future__ import annotations

import numpy as np

from .models import Model, select_weights

ORDER_ALL = "bgnmrv"      # OptX$p1..p6: brt, gam, nn, mars, rf, svm (V73:326-331)
ORDER_SMOOTH = "gnmv"     # smooth.outputs.only = TRUE (V73:366-372)


def holdout_rows(kfolds, v: int, n_rows: int):
    """V73:228-232: with more than 4000 rows the model is TRAINED on fold v and tested on the other nine."""
    kfolds = np.asarray(kfolds)
    return np.flatnonzero(kfolds != v) if n_rows > 4000 else np.flatnonzero(kfolds == v)


def train_rows(kfolds, v: int, n_rows: int):
    """The complement of :func:`holdout_rows` (V73:228-232): fold v itself when there are more than 4000 rows."""
    kfolds = np.asarray(kfolds)
    return np.flatnonzero(kfolds == v) if n_rows > 4000 else np.flatnonzero(kfolds != v)


def fit_linear_folds(X, resp, kfolds):
    """``mod.gam.tps.elev <- mgcv::gam(mod.form, data = train)`` for every fold (V73:252) on the device: the one
    member whose fit is deterministic (least squares, :meth:`models.Gam.fit`).  Returns the fold models in fold
    order, ready for the ``g`` slot of ``fold_models`` in :func:`cv_residuals`."""
    from .models import Gam
    X = np.asarray(X, dtype=np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    out = []
    for v in range(1, int(np.max(kfolds)) + 1):
        tr = train_rows(kfolds, v, X.shape[0])
        out.append(Gam.fit(X[tr], resp[tr]))
    return out


def fit_forest_folds(X, resp, kfolds, n_trees=500, mtry=None, nodesize=5, inbag=None, seeds=None, seed=0):
    """``mod.rf.tps.elev <- randomForest::randomForest(mod.form, data = train)`` for every fold (V73:248), ALL fold
    forests in ONE device call (:func:`models.rf_fit_many`: a workgroup per tree, folds x n_trees trees in one launch).
    Fold v is trained on :func:`train_rows`, so the > 4000-row rule of V73:228-232 holds.  ``inbag`` / ``seeds``: one
    array per fold (over that fold's training rows); ``None`` draws fold v's from ``default_rng([seed, v - 1])``.
    Returns the fold models in fold order, ready for the ``r`` slot of ``fold_models`` in :func:`cv_residuals`."""
    from .models import rf_fit_many
    Xs, ys, gen = _fold_batch(X, resp, kfolds, seed)
    return rf_fit_many(Xs, ys, n_trees, mtry, nodesize, inbag, seeds, gen)


def fit_earth_folds(X, resp, kfolds, nfold=10, seed=0, nk=None, thresh=0.001, penalty=2.0, minspan=0, endspan=0):
    """``mod.mars.tps.elev <- earth::earth(mod.form, data = train, nfold = 10)`` for every fold (V73:250), ALL fold
    models in ONE device call (:func:`models.earth_fit_many`: a workgroup per model); with ``nfold > 0`` that call covers
    folds x (1 + nfold) models, the sub-models behind every fold model's ``.cv_rsq``.  Fold v is trained on
    :func:`train_rows`, so the > 4000-row rule of V73:228-232 holds.  Fold v's sub-model folds come from
    ``default_rng([seed, v - 1])``.  Returns the fold models in fold order, ready for the ``m`` slot of ``fold_models`` in
    :func:`cv_residuals`."""
    from .models import earth_fit_many
    Xs, ys, gen = _fold_batch(X, resp, kfolds, seed)
    return earth_fit_many(Xs, ys, nk, thresh, penalty, minspan, endspan, nfold, None, gen)


def _fold_batch(X, resp, kfolds, seed):
    """the training rows of every fold (:func:`train_rows`) and what seeds fold v's generator: ``[seed, v - 1]``"""
    X = np.asarray(X, dtype=np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    nfolds = int(np.max(kfolds))
    rows = [train_rows(kfolds, v, X.shape[0]) for v in range(1, nfolds + 1)]
    gen = [[int(seed), v] for v in range(nfolds)] if np.ndim(seed) == 0 else list(seed)
    return [X[r] for r in rows], [resp[r] for r in rows], gen


def fit_nnet_folds(X, resp, kfolds, wts0=None, seed=0, maxit=10000):
    """``mod.nn.tps.elev <- nnet::nnet(mod.form, data = trainNN, size = 10, linout = TRUE, maxit = 10000)`` for every fold
    (V73:249) with the fold's own response scaling (V73:235-241), ALL fold models in ONE launch
    (:func:`models.nnet_fit_many`: a workgroup per model).  Fold v is trained on :func:`train_rows`, so the > 4000-row
    rule of V73:228-232 holds.  ``wts0``: one vector of initial weights per fold; ``None`` draws fold v's from
    ``default_rng([seed, v - 1]).uniform(-0.7, 0.7)``.  Returns the fold models in fold order, ready for the ``n`` slot
    of ``fold_models`` in :func:`cv_residuals`."""
    from .models import nnet_fit_many
    Xs, ys, gen = _fold_batch(X, resp, kfolds, seed)
    return nnet_fit_many(Xs, ys, wts0, gen, maxit=maxit)


def fit_ksvm_folds(X, resp, kfolds, sigma=None, seed=0):
    """``mod.svm.tps.elev <- kernlab::ksvm(mod.form, data = train)`` for every fold (V73:251), ALL fold models in ONE
    device call (:func:`models.ksvm_fit_many`: the SMO a workgroup per model).  Fold v is trained on :func:`train_rows`,
    so the > 4000-row rule of V73:228-232 holds.  ``sigma``: a scalar, one value per fold, or ``None`` -- kernlab's
    automatic width, fold v's from ``sigest(train, seed = [seed, v - 1])``.  Returns the fold models in fold order, ready
    for the ``v`` slot of ``fold_models`` in :func:`cv_residuals`."""
    from .models import ksvm_fit_many
    Xs, ys, gen = _fold_batch(X, resp, kfolds, seed)
    return ksvm_fit_many(Xs, ys, sigma, gen)


def kfold(n, k=10, seed=0):
    """``machisplin.kfold(x, k)`` (V73:1553-1573): 1-based fold labels for n rows.  The group sizes are the differences
    of ``round(c(0, n / k * 1:(k - 1), n))`` (R rounds half to even, as numpy does); the labels ``rep(j, times[j])`` are
    then put in a random order -- here a permutation from ``default_rng(seed)``, NOT R's ``order(runif(n))``."""
    n, k = int(n), int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    if k == 1:
        return np.ones(n, dtype=np.int64)
    if n / k < 1:
        raise ValueError("insufficient records: %d, with k = %d" % (n, k))
    edges = np.round(np.concatenate([[0.0], n / k * np.arange(1, k), [float(n)]])).astype(np.int64)
    group = np.repeat(np.arange(1, k + 1), np.diff(edges))
    return group[np.random.default_rng(seed).permutation(n)]


_MEMBER = {lab: i for i, lab in enumerate(ORDER_ALL)}


def _member_seeds(seed, lab, count):
    """``[seed, member, j]`` for j = 0 .. count - 1; member = the label's place in "bgnmrv" """
    return [[int(seed), _MEMBER[lab], j] for j in range(count)]


def _member_int_seed(seed, lab, j):
    """an int from the stream ``[seed, member, j]`` for :func:`gbm_step`, which takes an int and derives its own streams"""
    return int(np.random.SeedSequence([int(seed), _MEMBER[lab], j]).generate_state(1)[0])


def fit_layer(X, resp, kfolds=None, seed=0, smooth_only=False, nfolds=10, gbm_fold=None, gbm_final=None, rf=None, earth=None,
              nnet=None, ksvm=None, var_imp=False):
    """Step 1 and the final fits of ONE response layer (V73:220-620), every fit on the device:

    1. the fold labels: ``kfolds`` as given (1-based, one per row) or :func:`kfold` ``(n, nfolds, seed)`` (V73:220);
    2. the fold models of every member in play -- ``bgnmrv``, or ``gnmv`` with ``smooth_only`` (no tree is fitted then):
       ``b`` by :func:`gbm_step` fold by fold (``tree_complexity = 25, learning_rate = 0.01, bag_fraction = 0.5``,
       V73:247; ``gbm_fold`` overrides; an abort of machisplin.gbm.step raises ``RuntimeError`` naming the fold, as R
       stops there), the other five through :func:`fit_linear_folds`, :func:`fit_nnet_folds`, :func:`fit_earth_folds`,
       :func:`fit_forest_folds` and :func:`fit_ksvm_folds`, one device call per member; the dicts ``rf``, ``earth``,
       ``nnet`` and ``ksvm`` are forwarded to them as keywords;
    3. :func:`cv_residuals`, :func:`optx_weights`: the kept labels, their rounded weights, the unrounded total (V73:322-392);
    4. the final fits on ALL rows of the kept members only, in ``mods.run`` order (V73:447-619): ``b`` by
       :func:`gbm_step` with ``tree_complexity = 5, learning_rate = 0.001`` (V73:493; ``gbm_final`` overrides), ``n`` with
       the all-rows response scaling of V73:454-459, ``n`` and ``v`` through :func:`models.nnet_fit_many` /
       :func:`models.ksvm_fit_many`; the scalar arguments of the member's dict apply (a per-fold ``wts0``, ``inbag``,
       ``seeds`` or ``sigma`` sequence does not).

    Every draw comes from a ``default_rng`` stream derived from ``seed``, the member and the fold, none from R's: member
    ``bgnmrv`` is number 0 .. 5; fold v (1-based) of a member draws from ``default_rng([seed, member, v - 1])``, its final
    fit from ``default_rng([seed, member, nfolds])``; :func:`gbm_step` takes an int seed, which is the first word of
    ``SeedSequence([seed, 0, j])``; the fold labels come from ``default_rng(seed)``.  A ``seed`` in a member's dict
    replaces that member's derivation for the folds.  The same arguments give bit-identical results.

    ``var_imp = True`` adds the layer's ``$var.imp`` (V73:465 ... 602), a dict by kept label of one entry per predictor,
    in predictor order: ``b`` :meth:`models.Gbm.contributions` (percent), ``g`` the p slope coefficients (the intercept
    stays in the model's ``coefficients[0]``), ``n`` :func:`varimp.garson`, ``m`` :func:`varimp.evimp` as p x 3 (nsubsets,
    gcv, rss), ``r`` the forest's ``.importance`` (p x 2: raw %IncMSE, IncNodePurity; :func:`models.rf_importance_many`)
    and ``v`` :func:`varimp.ksvm_contributions`.  The forest's permutation seeds come from
    ``default_rng([seed, 4, nfolds, 1])`` and the ksvm sample from ``default_rng([seed, 5, nfolds, 1])``: streams of
    their own, so every other draw -- and every other entry of the result -- is the same bit for bit with and without it.

    Returns a dict: ``kfolds``, ``fold_models`` (per fold, label -> model), ``residuals`` (hold-out rows x members in
    play), ``p`` (the optimiser's end point), ``labels`` (the kept ones), ``models`` / ``weights`` / ``wt_total`` --
    exactly a ``fitted[i]`` of :func:`mltps.mltps` -- and, when asked for, ``var_imp``."""
    from . import models as _models
    X = np.ascontiguousarray(X, dtype=np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    n = X.shape[0]
    if X.ndim != 2 or resp.shape != (n,):
        raise ValueError("X must be n x p with one response per row")
    if kfolds is None:
        kfolds = kfold(n, nfolds, seed)
    else:
        kfolds = np.asarray(kfolds)
        if kfolds.shape != (n,):
            raise ValueError("kfolds needs one label per row")
    nf = int(np.max(kfolds))
    labels = ORDER_SMOOTH if smooth_only else ORDER_ALL
    nnet, ksvm, rf, earth = dict(nnet or {}), dict(ksvm or {}), dict(rf or {}), dict(earth or {})

    def with_seed(lab, kw):
        return {"seed": _member_seeds(seed, lab, nf), **kw}

    def run_gbm_step(Xt, yt, j, what, defaults, over):
        kw = {"seed": _member_int_seed(seed, "b", j), **defaults, "bag_fraction": 0.5, **(over or {})}
        res = gbm_step(Xt, yt, **kw)
        if res is None:
            raise RuntimeError("machisplin.gbm.step aborted for %s: restart with a smaller learning rate" % what)
        return res[0]

    by_label = {"g": fit_linear_folds(X, resp, kfolds),
                "n": fit_nnet_folds(X, resp, kfolds, **with_seed("n", nnet)),
                "m": fit_earth_folds(X, resp, kfolds, **with_seed("m", earth)),
                "v": fit_ksvm_folds(X, resp, kfolds, **with_seed("v", ksvm))}
    if not smooth_only:
        by_label["r"] = fit_forest_folds(X, resp, kfolds, **with_seed("r", rf))
        by_label["b"] = []
        for v in range(1, nf + 1):
            tr = train_rows(kfolds, v, n)
            by_label["b"].append(run_gbm_step(X[tr], resp[tr], v - 1, "fold %d" % v, {"tree_complexity": 25, "learning_rate": 0.01},
                                              gbm_fold))
    fold_models = [{lab: by_label[lab][v] for lab in labels} for v in range(nf)]
    residuals = cv_residuals(fold_models, X, resp, kfolds, labels)
    p_opt, kept, wts, tot = optx_weights(residuals, smooth_only)
    scalars = lambda kw, drop: {k: v for k, v in kw.items() if k not in drop}
    final = []
    for lab in kept:
        gen = [int(seed), _MEMBER[lab], nf]
        if lab == "b":
            m = run_gbm_step(X, resp, nf, "the final model", {"tree_complexity": 5, "learning_rate": 0.001}, gbm_final)
        elif lab == "g":
            m = _models.Gam.fit(X, resp)
        elif lab == "n":
            m = _models.nnet_fit_many([X], [resp], None, [gen], **scalars(nnet, ("wts0", "seed")))[0]
        elif lab == "m":       # (the *_fit_many take one seed PER MODEL: [gen] names the stream, a bare gen would be read as a list of them)
            m = _models.earth_fit_many([X], [resp], **{"nfold": 10, **scalars(earth, ("seed",)), "seed": [gen]})[0]
        elif lab == "r":
            m = _models.rf_fit_many([X], [resp], **{**scalars(rf, ("inbag", "seeds", "seed")), "seed": [gen]})[0]
        else:
            sig = ksvm.get("sigma")
            m = _models.ksvm_fit_many([X], [resp], sig if sig is None or np.ndim(sig) == 0 else None, [gen])[0]
        final.append(m)
    out = {"kfolds": kfolds, "fold_models": fold_models, "residuals": residuals, "p": p_opt, "labels": kept, "models": final,
           "weights": wts, "wt_total": tot}
    if var_imp:
        out["var_imp"] = {lab: _member_var_imp(lab, m, X, resp, [int(seed), _MEMBER[lab], nf, 1]) for lab, m in zip(kept, final)}
    return out


def _member_var_imp(lab, m, X, resp, gen):
    """the $var.imp entry of one final model (V73:465 ... 602); ``gen`` seeds what the entry draws"""
    from . import models as _models, varimp
    if lab == "b":
        return m.contributions()[0]
    if lab == "g":
        return m.coefficients[1:].copy()
    if lab == "n":
        return varimp.garson(m.wts, m.p, (m.wts.size - 1) // (m.p + 2))
    if lab == "m":
        return np.column_stack(varimp.evimp(m, m.p)[:3]).astype(np.float64)
    if lab == "r":
        seeds = np.random.default_rng(gen).integers(0, 2 ** 64, size=m.n_trees, dtype=np.uint64)
        return _models.rf_importance_many([m], [X], [resp], perm_seeds=[seeds])[0].importance
    return varimp.ksvm_contributions(m, X, seed=gen)


def cv_residuals(fold_models, X, resp, kfolds, labels: str = ORDER_ALL):
    """mfit.<model>.full of V73:258-319: for fold v = 1..nfolds, ``test$resp - predict(model_v, test)`` on the
    hold-out rows, concatenated in fold order.  ``fold_models[v-1]`` maps a label in ``labels`` to the device
    model (:class:`machisplin_amd.models.Model`) fitted on fold v's training rows; ``X`` is the n x p predictor
    matrix (covariates, LONG, LAT), ``kfolds`` the 1-based fold label of every row.
    Returns an (n_holdout_total, len(labels)) float64 matrix, columns in ``labels`` order."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    cols = {lab: [] for lab in labels}
    for v, models in enumerate(fold_models, start=1):
        rows = holdout_rows(kfolds, v, X.shape[0])
        Xt = np.ascontiguousarray(X[rows])
        for lab in labels:
            m = models[lab]
            if not isinstance(m, Model):
                raise TypeError("fold %d: model %r is not a device model" % (v, lab))
            cols[lab].append(resp[rows] - m.predict_points(Xt))
    return np.column_stack([np.concatenate(cols[lab]) for lab in labels])


def optx_objective(k, gram):
    """machisplin.optimx.internal (V73:329-331, 369-371) through the Gram matrix of the residual columns."""
    k = np.asarray(k, dtype=np.float64)
    s = k.sum()
    return float(k @ gram @ k) / (s * s)


def optx_weights(residuals, smooth_only: bool = False):
    """OptX of V73:333 / 373: minimise the objective from par = 0.5 in [0, 1]^m with L-BFGS-B (numerical
    gradient, as optimx does without ``gr``), then apply V73:336-362.  Returns (p, kept labels, kept rounded
    weights, unrounded total)."""
    from scipy.optimize import minimize
    R = np.asarray(residuals, dtype=np.float64)
    labels = ORDER_SMOOTH if smooth_only else ORDER_ALL
    if R.ndim != 2 or R.shape[1] != len(labels):
        raise ValueError("residuals must have %d columns (%s)" % (len(labels), labels))
    gram = R.T @ R
    res = minimize(optx_objective, np.full(len(labels), 0.5), args=(gram,), method="L-BFGS-B",
                   bounds=[(0.0, 1.0)] * len(labels))
    kept, wts, tot = select_weights(res.x, labels)
    return res.x, kept, wts, tot


def gbm_step_search(fold_models, X, y, selector, step: int = 50, tolerance: float = 0.001, max_trees: int = 10000,
                    site_weights=None):
    """The tree-count search of ``machisplin.gbm.step`` (V73:1765-1981) over fold models that gbm has grown far enough
    (grown by gbm in R, or by :func:`models.gbm_fit_many`; :func:`gbm_step` does both the growing and this search):

    * fold i's model predicts its hold-out rows (``selector == i``) at n.trees = step, 2 step, ... in ONE device walk
      (:meth:`models.Gbm.staged_predict_points`; R calls predict.gbm once per stage, V73:1843, 1919);
    * ``cv.loss.values[j]`` = mean over the folds of the hold-out deviance, gaussian = mean squared error
      (machisplin.calc.deviance, V73:2250-2285; V73:1866, 1942-1946);
    * stages are added while ``delta.deviance > tolerance.test`` and ``n.fitted < max.trees`` (V73:1884); from the
      20th stage on ``delta.deviance = mean(cv[j-19 .. j-9]) - mean(cv[j-9 .. j])`` (V73:1957-1961);
      ``tolerance.test`` = tolerance x the mean total deviance (tolerance.method = "auto", V73:1786-1794);
    * a loss that rises within the first four stages aborts (V73:1948-1955: returns None, R prints "restart model
      with a smaller learning rate");
    * the tree count is the first stage with the smallest loss (V73:1976-1981).

    Returns ``(target_trees, cv_loss_values, trees_fitted)``."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    selector = np.asarray(selector)
    w = np.ones_like(y) if site_weights is None else np.asarray(site_weights, dtype=np.float64)
    u = np.sum(y * w) / np.sum(w)
    tolerance_test = float(np.sum((y - u) * (y - u))) / y.size * tolerance
    staged = []
    for i, m in enumerate(fold_models):
        mask = selector == i + 1
        P = m.staged_predict_points(X[mask], step)
        d = y[mask][None, :] - P
        staged.append(np.sum(d * d, axis=1) / int(mask.sum()))

    def stage_loss(j):
        if j > len(staged[0]):
            raise ValueError("fold models have fewer trees than the search needs")
        return float(np.mean([s[j - 1] for s in staged]))
    return _gbm_step_rule(stage_loss, tolerance_test, step, step, max_trees)


def _gbm_step_rule(stage_loss, tolerance_test, first: int, step: int, max_trees: int):
    """The stopping rule of machisplin.gbm.step (V73:1872-1981) shared by :func:`gbm_step_search` and :func:`gbm_step`:
    ``stage_loss(j)`` is cv.loss.values[j] (j = 1: after the first ``first`` trees, then ``step`` more per stage), asked
    for stage by stage.  Returns ``(target_trees, cv_loss_values, trees_fitted)`` or None on the early-rise abort."""
    n_fitted = first
    trees = [n_fitted]
    cv = [stage_loss(1)]
    delta, j = 1.0, 1
    while delta > tolerance_test and n_fitted < max_trees:
        n_fitted += step
        trees.append(n_fitted)
        j += 1
        cv.append(stage_loss(j))
        if j < 5 and cv[j - 1] > cv[j - 2]:
            return None
        if j >= 20:
            delta = float(np.mean(cv[j - 20:j - 9]) - np.mean(cv[j - 10:j]))
    cv = np.array(cv)
    return trees[int(np.argmax(cv == cv.min()))], cv, np.array(trees)


def gbm_step(X, y, fold_vector=None, seed=0, tree_complexity=25, learning_rate=0.01, bag_fraction=0.5, n_folds=10,
             n_trees=50, step_size=50, max_trees=10000, tolerance=0.001, n_minobsinnode=10):
    """``machisplin.gbm.step(tree.complexity = 25, learning.rate = 0.01, bag.fraction = 0.5)`` (V73:247, V73:493;
    gaussian, no site weights, no prevalence stratification) with the growing on the device:

    * the selector is ``fold_vector`` (1-based fold labels) or, as V73:1748-1749, ``rep(1 .. n_folds, length = n)`` in
      a random order -- here a permutation from ``numpy.random.default_rng(seed)``, not R's ``runif`` stream;
    * the ``n_folds`` fold models (fold i trained on ``selector != i``) grow ``n_trees`` trees (V73:1772), then
      ``step_size`` more per stage (gbm.more, V73:1908), ALL folds in one device call per stage
      (:func:`models.gbm_fit_many` / :func:`models.gbm_more_many`); fold i's bags come from ``default_rng([seed, i])``;
    * after every stage each fold model predicts its hold-out rows (:meth:`models.Model.predict_points`) and the mean
      hold-out deviance joins the loss curve; the stopping rule is the one of :func:`gbm_step_search`;
    * the final model is grown on all rows with ``target_trees`` trees (V73:2101), bags from ``default_rng([seed, n_folds])``.

    Returns ``(final_model, target_trees, cv_loss_values, trees_fitted)`` -- the final model also carries
    ``.fold_vector`` and ``.fold_models`` (as grown when the search stopped) -- or None on the early-rise abort."""
    from . import models as _models
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    if fold_vector is None:
        selector = np.resize(np.arange(1, n_folds + 1), n)[np.random.default_rng(seed).permutation(n)]
    else:
        selector = np.asarray(fold_vector)
        if selector.size != n:
            raise ValueError("fold_vector needs one label per row")
        n_folds = int(selector.max())
    tolerance_test = float(np.sum((y - y.mean()) * (y - y.mean()))) / n * tolerance
    hold = [np.flatnonzero(selector == i + 1) for i in range(n_folds)]
    train = [np.flatnonzero(selector != i + 1) for i in range(n_folds)]
    Xh = [np.ascontiguousarray(X[h]) for h in hold]
    state = {"folds": None}

    def stage_loss(j):
        if j == 1:
            state["folds"] = _models.gbm_fit_many([X[t] for t in train], [y[t] for t in train], n_trees, None,
                                                  [[int(seed), i] for i in range(n_folds)], tree_complexity, learning_rate,
                                                  bag_fraction, n_minobsinnode)
        else:
            state["folds"] = _models.gbm_more_many(state["folds"], step_size)
        loss = []
        for m, h, xh in zip(state["folds"], hold, Xh):
            d = y[h] - m.predict_points(xh)
            loss.append(np.sum(d * d) / h.size)
        return float(np.mean(loss))

    res = _gbm_step_rule(stage_loss, tolerance_test, n_trees, step_size, max_trees)
    if res is None:
        return None
    target, cv, trees = res
    final = _models.gbm_fit_many([X], [y], target, None, [[int(seed), n_folds]], tree_complexity, learning_rate, bag_fraction,
                                 n_minobsinnode)[0]
    final.fold_vector, final.fold_models = selector, state["folds"]
    return final, target, cv, trees
