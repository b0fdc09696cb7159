"""GPU: gbm's boosted trees grown on the device (mhs_gbm_grow_many through models.Gbm.fit / gbm_fit_many / cv.gbm_step)
against the numpy reference of the growth rule (tests/gbm_ref.py).  test_gbm_ref_host.py shows that the structures of
these inputs do not hinge on the summation order, which is what makes the exact structural comparisons fair."""
import subprocess
import sys

import numpy as np
import pytest

import gbm_inputs as gi
import gbm_ref
from oracle import ensemble as oe
from oracle import fit as of


def _trees(params):
    return [gbm_ref.tree_of(params, t) for t in range(len(params["tree_offsets"]) - 1)]


def _slice(params, t0, t1):
    """trees t0 .. t1-1 of a bundle as a bundle of their own with init_f = 0"""
    off = params["tree_offsets"]
    sub = {k: params[k][off[t0]:off[t1]] for k in ("split_var", "split_val", "left", "right", "missing")}
    sub.update(kind="gbm", init_f=0.0, tree_offsets=off[t0:t1 + 1] - off[t0], p=params["p"])
    return sub


def _bit_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in
               ("tree_offsets", "split_var", "split_val", "left", "right", "missing")) and a["init_f"] == b["init_f"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["short", "stations"])
def test_exact_against_the_reference(hip, name):
    """40 bagged trees, depth 25, learning rate 0.01: every tree's split variables, split values (bit-equal) and
    topology equal the reference's; terminal values and the fit agree to 1e-12 max|y|."""
    X, y, bags = getattr(gi, name)()
    m = hip.models.Gbm.fit(X, y, 40, bags=bags)
    ref, F, rtrees = gbm_ref.fit(X, y, 40, bags)
    tol = 1e-12 * np.abs(y).max()
    same = [gbm_ref.same_structure(a, b) for a, b in zip(_trees(m.params), rtrees)]
    print(name, "identical trees", sum(same), "/ 40; max |fit - ref|", np.abs(m.fit - F).max(), "init_f diff", abs(m.init_f - ref["init_f"]))
    assert all(same)
    assert np.array_equal(m.params["tree_offsets"], ref["tree_offsets"])
    term = ref["split_var"] < 0
    assert np.abs(m.params["split_val"][term] - ref["split_val"][term]).max() <= tol
    assert np.array_equal(m.params["split_val"][~term], ref["split_val"][~term])
    assert abs(m.init_f - ref["init_f"]) <= tol
    assert np.abs(m.fit - F).max() <= tol


def _teacher_forced(model, X, y, bags, compared):
    """For every tree t in ``compared`` (1-based): F from the device's first t - 1 trees (the oracle's evaluator), the
    reference's tree t from that F and the same bag, compared whole with the device's.  Returns (compared, differing,
    differing trees that are not near-ties of the reference)."""
    orders = gbm_ref.sort_orders(X)
    p = model.params
    n_cmp = n_diff = n_bad = 0
    for t in compared:
        sub = dict(p)
        sub["tree_offsets"] = p["tree_offsets"][:t]
        z = y - oe.predict(sub, X)
        ref = gbm_ref.grow_tree(X, z, bags[t - 1], orders, 25, 10, 0.01)
        dev = gbm_ref.tree_of(p, t - 1)
        n_cmp += 1
        term = ref["split_var"] < 0
        if not gbm_ref.same_structure(ref, dev) or np.abs(dev["split_val"][term] - ref["split_val"][term]).max() > 1e-12 * np.abs(y).max():
            n_diff += 1
            n_bad += not (not gbm_ref.same_structure(ref, dev) and gbm_ref.near_tie(X, z, ref, dev, 10, 1e-9))
    return n_cmp, n_diff, n_bad


@pytest.mark.gpu
def test_teacher_forced_long(hip):
    """10 models in one call, n = 3600, p = 7, 500 trees, bag 0.5: every 25th tree equals the reference's tree grown
    from the device's own F; a tree may differ only on a near-tie of the reference's improvements (1e-9 relative), and
    such trees are at most 2 % of those compared."""
    data = gi.long_models()
    models = hip.models.gbm_fit_many([d[0] for d in data], [d[1] for d in data], 500, bags=[d[2] for d in data])
    tot = diff = bad = 0
    for m, (X, y, bags) in zip(models, data):
        c, d, b = _teacher_forced(m, X, y, bags, range(gi.LONG_EVERY, 501, gi.LONG_EVERY))
        tot, diff, bad = tot + c, diff + d, bad + b
    print("teacher-forced: compared", tot, "differing", diff, "not near-ties", bad)
    assert bad == 0
    assert diff <= 0.02 * tot


@pytest.mark.gpu
def test_teacher_forced_large_n(hip):
    """n = 20 000 (the rows no longer fit on chip): 5 sampled trees pass the teacher-forced check"""
    X, y, bags = gi.large()
    m = hip.models.Gbm.fit(X, y, bags.shape[0], bags=bags)
    c, d, b = _teacher_forced(m, X, y, bags, gi.LARGE_SAMPLED)
    print("large n: compared", c, "differing", d, "not near-ties", b)
    assert b == 0 and d <= 0.02 * c
    assert np.abs(m.predict_points(X) - m.fit).max() <= 1e-11 * np.abs(y).max()


@pytest.mark.gpu
def test_consistent_with_the_evaluator(hip):
    X, y, bags = gi.short()
    m = hip.models.Gbm.fit(X, y, 40, bags=bags)
    tol = 1e-11 * np.abs(y).max()
    assert np.abs(m.predict_points(X) - m.fit).max() <= tol
    assert np.abs(oe.predict(m.params, X) - m.fit).max() <= tol
    X2, y2, b2 = gi.stations()
    m2 = hip.models.Gbm.fit(X2, y2, 40, bags=b2)
    tol2 = 1e-11 * np.abs(y2).max()
    assert np.abs(m2.predict_points(X2) - m2.fit).max() <= tol2
    assert np.abs(oe.predict(m2.params, X2) - m2.fit).max() <= tol2


def _check_invariants(params, X, y, bags, F0, depth, minobs, shrinkage):
    """Walk every tree with its bag rows: <= depth splits, left / right terminals with >= minobs bag rows, missing
    children with the parent's mean, splits strictly between distinct data values of the node."""
    F = np.full(y.size, F0)
    for t, tr in enumerate(_trees(params)):
        var, val, left, right, miss = (tr[k] for k in ("split_var", "split_val", "left", "right", "missing"))
        assert np.sum(var >= 0) <= depth and var.size == 3 * np.sum(var >= 0) + 1
        z = y - F
        stack = [(0, np.asarray(bags[t]))]
        while stack:
            e, rows = stack.pop()
            mean = z[rows].mean()
            if var[e] < 0:
                assert rows.size >= minobs or e == 0
                assert abs(val[e] - shrinkage * mean) <= 1e-12 * np.abs(y).max()
                continue
            x = X[rows, var[e]]
            lo, hi = x[x < val[e]], x[x >= val[e]]
            assert lo.size >= minobs and hi.size >= minobs
            assert lo.max() < val[e] < hi.min()
            assert var[miss[e]] < 0 and abs(val[miss[e]] - shrinkage * mean) <= 1e-12 * np.abs(y).max()
            stack += [(left[e], rows[x < val[e]]), (right[e], rows[x >= val[e]])]
        F = F + gbm_ref.tree_values(tr, X)
    return F


@pytest.mark.gpu
def test_invariants(hip):
    X, y, bags = gi.short()
    for depth, minobs in ((25, 10), (3, 10), (25, 1), (6, 40)):
        m = hip.models.Gbm.fit(X, y, 12, bags=bags[:12], interaction_depth=depth, n_minobsinnode=minobs, shrinkage=0.05)
        F = _check_invariants(m.params, X, y, bags, m.init_f, depth, minobs, 0.05)
        assert np.abs(F - m.fit).max() <= 1e-12 * np.abs(y).max()
    X2, y2, b2 = gi.stations()
    m2 = hip.models.Gbm.fit(X2, y2, 10, bags=b2[:10])
    _check_invariants(m2.params, X2, y2, b2, m2.init_f, 25, 10, 0.01)
    # constant response: root-only trees
    mc = hip.models.Gbm.fit(X, np.full(300, 2.5), 5, bags=bags[:5])
    assert np.array_equal(mc.params["tree_offsets"], np.arange(6)) and np.all(mc.params["split_var"] == -1)
    assert np.all(mc.fit == 2.5)
    # a bag smaller than 2 n.minobsinnode: no candidate split
    ms = hip.models.Gbm.fit(X, y, 5, bags=bags[:5, :19])
    assert np.array_equal(ms.params["tree_offsets"], np.arange(6)) and np.all(ms.params["split_var"] == -1)
    assert np.any(ms.params["split_val"] != 0.0)


@pytest.mark.gpu
def test_reproducible(hip):
    data = gi.long_models(count=10, n_trees=100)
    Xs, ys, bs = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
    a = hip.models.gbm_fit_many(Xs, ys, 100, bags=bs)
    b = hip.models.gbm_fit_many(Xs, ys, 100, bags=bs)
    for u, v in zip(a, b):
        assert _bit_equal(u.params, v.params) and np.array_equal(u.fit, v.fit)
    alone = hip.models.Gbm.fit(Xs[3], ys[3], 100, bags=bs[3])
    assert _bit_equal(alone.params, a[3].params) and np.array_equal(alone.fit, a[3].fit)
    half = hip.models.Gbm.fit(Xs[3], ys[3], 50, bags=bs[3][:50]).more(50, bags=bs[3][50:])
    assert half.n_trees == 100
    assert _bit_equal(half.params, alone.params) and np.array_equal(half.fit, alone.fit)
    # models of different sizes in one call, seeded bags: the same trees as each alone
    mixed = hip.models.gbm_fit_many([Xs[0][:700], Xs[1]], [ys[0][:700], ys[1]], 20, seed=[5, 6])
    solo = hip.models.Gbm.fit(Xs[0][:700], ys[0][:700], 20, seed=5)
    assert _bit_equal(mixed[0].params, solo.params)
    again = solo.more(10)
    assert again.n_trees == 30 and np.abs(again.predict_points(Xs[0][:700]) - again.fit).max() <= 1e-11 * np.abs(ys[0]).max()


@pytest.mark.gpu
def test_gbm_step(hip):
    """cv.gbm_step on n = 600: the tree count, the loss curve and trees_fitted are what the oracle's stopping rule
    gives on hold-out curves computed with the oracle's evaluator from the device's own fold models."""
    rng = np.random.default_rng(21)
    n = 600
    X = rng.normal(size=(n, 5))
    y = 3.0 * np.sin(X[:, 0]) + X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=n)
    fold_vector = np.resize(np.arange(1, 11), n)[np.random.default_rng(22).permutation(n)]
    res = hip.cv.gbm_step(X, y, fold_vector=fold_vector, seed=3, learning_rate=0.05, max_trees=3000)
    assert res is not None
    final, target, cv, trees = res
    staged = []
    for i, fm in enumerate(final.fold_models):
        mask = fold_vector == i + 1
        pred, curve = np.full(int(mask.sum()), fm.params["init_f"]), []
        for k in range(fm.n_trees // 50):                  # the oracle's evaluator, 50 trees at a time
            pred = pred + oe.predict(_slice(fm.params, 50 * k, 50 * (k + 1)), X[mask])
            curve.append(of.gaussian_deviance(y[mask], pred))
        staged.append(np.array(curve))
    tol_test = float(np.sum((y - y.mean()) ** 2)) / n * 0.001
    want = of.gbm_step_rule(staged, tol_test, 50, 3000)
    print("gbm_step: target", target, "stages", len(cv), "oracle target", want[0])
    assert target == want[0]
    assert np.array_equal(trees, want[2])
    assert np.allclose(cv, want[1], rtol=1e-9, atol=0)
    assert final.n_trees == target and len(final.params["tree_offsets"]) == target + 1
    assert all(fm.n_trees == trees[-1] for fm in final.fold_models)
    assert np.abs(final.predict_points(X) - final.fit).max() <= 1e-11 * np.abs(y).max()


@pytest.mark.gpu
def test_errors(hip):
    from machisplin_amd import _lib
    X, y, bags = gi.short()
    Xn = X.copy()
    Xn[17, 2] = np.nan
    with pytest.raises(hip.MhsError) as ei:
        hip.models.Gbm.fit(Xn, y, 3, bags=bags[:3])
    assert ei.value.code == _lib.ERR_INVALID
    bad = bags[:3].copy()
    bad[1, 5] = 300
    with pytest.raises(hip.MhsError) as ei:
        hip.models.Gbm.fit(X, y, 3, bags=bad)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(hip.MhsError) as ei:
        hip.models.Gbm.fit(X[:100], y[:100], 3, bags=bags[:3] % 100)        # bag_size 150 > n = 100
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(hip.MhsError) as ei:
        hip.models.Gbm.fit(X[:, :1], y, 3, bags=bags[:3])                   # p below mhs_gbm_load's range
    assert ei.value.code == _lib.ERR_INVALID


_BEFORE_INIT = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from machisplin_amd import _lib
lib = _lib.load()
n, p, T, B, d = 50, 3, 2, 25, 4
X = np.asfortranarray(np.random.default_rng(0).normal(size=(n, p))); y = X[:, 0].copy()
bags = np.stack([np.arange(B, dtype=np.int32)] * T); F = np.zeros(n); init = np.zeros(1)
off = np.zeros(T + 1, dtype=np.int64); cap = T * (3 * d + 1)
iv = [np.zeros(cap, dtype=np.int32) for _ in range(4)]; val = np.zeros(cap)
pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
ns = np.array([n], dtype=np.int64); bs = np.array([B], dtype=np.int64)
rc = lib.mhs_gbm_grow_many(1, pa(X), pa(y), ns.ctypes.data, p, pa(bags), bs.ctypes.data, T, d, 10, 0.01, 1, pa(F), init.ctypes.data,
                           pa(off), pa(iv[0]), pa(val), pa(iv[1]), pa(iv[2]), pa(iv[3]))
sys.exit(0 if rc == _lib.ERR_NODEVICE else 1)
"""


def test_call_before_init_is_refused():
    """a fresh process that has not called mhs_init: MHS_ERR_NODEVICE (with or without a GPU in the machine)"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", _BEFORE_INIT, root], timeout=300).returncode == 0
