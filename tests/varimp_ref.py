"""Numpy restatements of the variable-importance rules (include/machisplin_hip.h, machisplin_amd/varimp.py), written from
the rules' statements and not from the code under test: the forest's permutation importance (walks by rf_ref.predict,
keys by rf_ref.mix, permutations by np.argsort(kind = "stable")), garson, evimp and breakDown's step-up."""
import numpy as np

import rf_ref

_M = (1 << 64) - 1


def permutation(seed, k, v, p, m):
    """sigma of tree seed ``seed``, permutation k, variable v over m out-of-bag rows: the stable ascending argsort of
    key_j = mix(mix(seed + k p + v) + j)"""
    h = rf_ref.mix((int(seed) + k * p + v) & _M)
    keys = np.array([rf_ref.mix((h + j) & _M) for j in range(m)], dtype=np.uint64)
    return np.argsort(keys, kind="stable")


def used_variables(tree, p):
    used = np.zeros(p, dtype=bool)
    used[np.asarray(tree["best_var"])[np.asarray(tree["status"]) != -1] - 1] = True
    return used


def tree_delta(tree, X, y, inbag_t, seed, n_perm):
    """delta[v] of one tree (a dict of tree-local arrays, rf_ref.tree_of): (mean_k e_k - e0) / m over its out-of-bag rows"""
    p = X.shape[1]
    O = np.flatnonzero(np.asarray(inbag_t) == 0)
    m = O.size
    out = np.zeros(p)
    if m == 0:
        return out
    XO, yO = X[O], y[O]
    e0 = float(np.sum((rf_ref.predict(tree, XO) - yO) ** 2))
    used = used_variables(tree, p)
    for v in range(p):
        if not used[v]:
            continue
        s = 0.0
        for k in range(n_perm):
            Xp = XO.copy()
            Xp[:, v] = XO[permutation(seed, k, v, p, m), v]
            s = s + float(np.sum((rf_ref.predict(tree, Xp) - yO) ** 2))
        out[v] = (s / n_perm - e0) / m
    return out


def forest_delta(params, X, y, inbag, perm_seeds, n_perm):
    """n_trees x p: tree_delta of every tree of a kind = "rf" bundle"""
    nt = len(params["tree_offsets"]) - 1
    return np.stack([tree_delta(rf_ref.tree_of(params, t), X, y, inbag[t], perm_seeds[t], n_perm) for t in range(nt)])


def inc_mse(delta):
    """(IncMSE, SD) from an n_trees x p array of deltas, summed in tree order"""
    nt, p = delta.shape
    s, s2 = np.zeros(p), np.zeros(p)
    for t in range(nt):
        s = s + delta[t]
        s2 = s2 + delta[t] * delta[t]
    mean = s / nt
    return mean, np.sqrt(np.maximum(0.0, (s2 / nt - mean * mean) / nt))


def garson(wts, p, size):
    """hidden unit h holds wts[h (p + 1)] (bias) and then its p input weights; the output's bias and the hidden weights follow"""
    w = np.asarray(wts, dtype=np.float64)
    imp = np.zeros(p)
    for h in range(size):
        q = np.array([abs(w[h * (p + 1) + 1 + i]) * abs(w[(p + 1) * size + 1 + h]) for i in range(p)])
        imp += q / q.sum()
    return imp / imp.sum()


def breakdown_up(predict, x_star, D):
    """(c, b0): breakDown's step-up with baseline = "intercept", one predict call per open variable and step"""
    D = np.array(D, dtype=np.float64)
    p = D.shape[1]
    b0 = b = float(np.mean(predict(D)))
    c = np.zeros(p)
    open_ = list(range(p))
    for _ in range(p):
        best, mu_best = None, 0.0
        for v in open_:
            T = D.copy()
            T[:, v] = x_star[v]
            mu = float(np.mean(predict(T)))
            if best is None or abs(mu - b) > abs(mu_best - b):
                best, mu_best = v, mu
        c[best] = mu_best - b
        b = mu_best
        D[:, best] = x_star[best]
        open_.remove(best)
    return c, b0
