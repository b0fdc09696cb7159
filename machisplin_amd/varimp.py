"""Variable importance of the ensemble members: what machisplin.mltps stores next to every final fit as the layer's
``$var.imp`` (V73:465 garson, V73:495 the gbm contributions, V73:517-519 randomForest's importance, V73:541 evimp,
V73:562-580 the breakDown loop for ksvm, V73:602 the gam coefficients) and ``machisplin.write.loadings`` prints
(V73:1082).  The two tree members' measures come from the device with the fit (:meth:`models.Gbm.contributions`,
:func:`models.rf_importance_many`); this module holds the host rules of the others, pure numpy on arrays: :func:`garson`,
:func:`evimp`, :func:`breakdown_up` -- and :func:`ksvm_contributions`, which drives the break-down of all its
observations through a handful of device calls."""
from __future__ import annotations

import numpy as np


def garson(wts, p, size):
    """NeuralNetTools' ``garson`` for one hidden layer and one output (V73:465), on nnet's weight vector: per hidden unit
    h its bias and then the p input weights w_ih, then the output's bias and the ``size`` hidden weights v_h.  The biases
    are ignored; ``Q_ih = |w_ih| |v_h|``, ``r_ih = Q_ih / sum_i Q_ih``, ``rel_imp_i = sum_h r_ih / sum_i sum_h r_ih``.
    Returns the p relative importances (they sum to 1).  A hidden unit whose Q are all zero contributes nothing."""
    w = np.asarray(wts, dtype=np.float64)
    p, size = int(p), int(size)
    if w.shape != ((p + 1) * size + size + 1,):
        raise ValueError("wts has the wrong length for (p, size)")
    w_in = w[:(p + 1) * size].reshape(size, p + 1)[:, 1:]           # size x p
    v = w[(p + 1) * size + 1:]                                      # size
    Q = np.abs(w_in) * np.abs(v)[:, None]
    tot = Q.sum(axis=1, keepdims=True)
    r = np.divide(Q, tot, out=np.zeros_like(Q), where=tot > 0.0)
    s = r.sum(axis=0)
    return s / s.sum()


def evimp(record, p):
    """earth's ``evimp`` (V73:541) on the record of a device fit (``mhs_earth_get``: the attributes of a fitted
    :class:`models.Earth`, or a dict of them -- ``forward["dirs"]``, ``prune_terms``, ``selected``, ``rss_per_subset``,
    ``gcv_per_subset``).  For the subset sizes k = 2 .. n_selected the variables with a non-zero ``dirs`` entry among the
    forward terms of ``prune_terms`` row k - 1 each get ``nsubsets += 1``, ``gcv += gcv_per_subset[k - 2] -
    gcv_per_subset[k - 1]`` and ``rss`` likewise; gcv and rss then become ``sign(x) sqrt(|x|)`` scaled so that the largest
    is 100 (earth's ``sqrt. = TRUE``).  Returns ``(nsubsets, gcv, rss, order)``: the three per-variable arrays in VARIABLE
    order and the variables in descending order of nsubsets, then gcv (ties to the lower index).  Parity with earth's
    ``evimp`` is NOT pinned, as the earth fit itself is not (include/machisplin_hip.h)."""
    rec = record if isinstance(record, dict) else vars(record)
    p = int(p)
    fdirs = np.asarray(rec["forward"]["dirs"])
    pt = np.asarray(rec["prune_terms"])
    gcv_sub, rss_sub = np.asarray(rec["gcv_per_subset"], dtype=np.float64), np.asarray(rec["rss_per_subset"], dtype=np.float64)
    n_selected = int(np.sum(np.asarray(rec["selected"], dtype=bool)))
    if fdirs.ndim != 2 or fdirs.shape[1] != p:
        raise ValueError("the record's dirs must be n_forward x p")
    nsub, gcv, rss = np.zeros(p, dtype=np.int64), np.zeros(p), np.zeros(p)
    for k in range(2, n_selected + 1):
        terms = pt[k - 1]
        used = np.any(fdirs[terms[terms >= 0]] != 0, axis=0)
        nsub[used] += 1
        gcv[used] += gcv_sub[k - 2] - gcv_sub[k - 1]
        rss[used] += rss_sub[k - 2] - rss_sub[k - 1]

    def scaled(x):
        x = np.sign(x) * np.sqrt(np.abs(x))
        top = x.max() if x.size else 0.0
        return 100.0 * x / top if top > 0.0 else x

    gcv, rss = scaled(gcv), scaled(rss)
    return nsub, gcv, rss, np.lexsort((np.arange(p), -gcv, -nsub))


def breakdown_up_many(predict, obs, D):
    """breakDown's step-up with baseline = "intercept" for every row of ``obs`` (m x p) against the data ``D`` (s x p);
    ``predict`` maps rows (k x p) to k predictions.  All observations advance together: per greedy step ONE ``predict``
    call over (observations x open variables x data rows), at most p of them after the one for the baseline.  Returns
    ``(C, b0)``: ``C[o, v]`` the contribution of variable v for observation o (see :func:`breakdown_up`), ``b0`` the
    baseline ``mean predict(D)``.  ``sum_v C[o, v] = mean predict(D with every column := obs[o]) - b0``."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    if obs.ndim != 2 or D.ndim != 2 or obs.shape[1] != D.shape[1] or D.shape[0] < 1:
        raise ValueError("obs and D must be matrices with the same columns")
    m, p = obs.shape
    s = D.shape[0]
    b0 = float(np.mean(np.asarray(predict(D), dtype=np.float64)))
    cur = np.broadcast_to(D, (m, s, p)).copy()              # every observation's data, the chosen columns replaced so far
    b = np.full(m, b0)
    C = np.zeros((m, p))
    open_ = np.ones((m, p), dtype=bool)
    for step in range(p):
        vs = np.nonzero(open_)[1].reshape(m, p - step)      # the open variables of every observation, ascending
        trial = np.repeat(cur[:, None, :, :], p - step, axis=1)                         # m x open x s x p
        oi, qi = np.meshgrid(np.arange(m), np.arange(p - step), indexing="ij")
        trial[oi, qi, :, vs] = obs[oi, vs][:, :, None]
        mu = np.asarray(predict(trial.reshape(-1, p)), dtype=np.float64).reshape(m, p - step, s).mean(axis=2)
        q = np.argmax(np.abs(mu - b[:, None]), axis=1)      # the first of equal maxima: the lowest variable
        rows = np.arange(m)
        v = vs[rows, q]
        C[rows, v] = mu[rows, q] - b
        b = mu[rows, q]
        cur[rows, :, v] = obs[rows, v][:, None]
        open_[rows, v] = False
    return C, b0


def breakdown_up(predict, x_star, D):
    """``breakDown::broken(model, new_observation = x_star, data = D, baseline = "intercept", direction = "up")`` as a
    rule: ``b = mean predict(D)``; p times: for every open variable v, ``mu_v = mean predict(D with column v := x*_v)``;
    the v with the largest ``|mu_v - b|`` (the lowest index on a tie) gets ``c_v = mu_v - b``, its column stays replaced
    and ``b = mu_v``.  Returns ``(c, b0)``: the p contributions in VARIABLE order and the baseline."""
    C, b0 = breakdown_up_many(predict, np.asarray(x_star, dtype=np.float64)[None, :], D)
    return C[0], b0


def ksvm_contributions(model, X, sample=200, seed=0, rows=None):
    """The ksvm member's $var.imp (the intent of V73:562-580): the mean over the sample rows of ``|c_v|``, the
    :func:`breakdown_up` contributions of each sample row against the sample itself, per variable.  The sample is
    ``rows`` (row indices of X), or all rows when ``n <= sample``, or ``default_rng(seed).choice(n, sample, replace =
    False)`` -- NOT R's ``sample``.  ``model``: anything with ``predict_points`` (a :class:`models.Ksvm`); all
    observations advance together, ONE ``predict_points`` call per greedy step (:func:`breakdown_up_many`).

    Two quirks of the reference loop are NOT reproduced: it counts its first observation twice (V73:572-573: both
    ``if`` lines run on the first pass), and it adds the rows of ``explain_z$contribution`` by GREEDY POSITION -- which
    differs from observation to observation -- not by variable, then labels them with the last observation's order.
    Returns the p mean absolute contributions in variable order."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be n x p")
    n = X.shape[0]
    if rows is None:
        rows = np.arange(n) if n <= int(sample) else np.random.default_rng(seed).choice(n, int(sample), replace=False)
    D = X[np.asarray(rows)]
    C, _ = breakdown_up_many(model.predict_points, D, D)
    return np.mean(np.abs(C), axis=0)
