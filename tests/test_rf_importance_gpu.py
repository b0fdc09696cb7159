"""GPU: randomForest's permutation importance on the device (mhs_rf_importance_many through models.rf_importance_many /
RandomForest.importance / RandomForest.fit(importance = True)) against the numpy restatement of the rule
(tests/varimp_ref.py) run on the device's OWN trees.

THE BOUND.  Walks and permutations are exact (comparisons of doubles, integer sorts), so device and restatement differ
only in the ORDER of the two sums of squares behind a delta.  Every |pred - y| <= R = max y - min y (a prediction is a
mean of responses); a sum of m non-negative terms in any order errs by at most m 2^-53 of itself, i.e. by m 2^-53 m R^2;
there are two such sums on either side, each divided by m: |delta_dev - delta_ref| <= 4 m_max 2^-53 R^2."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rf_inputs as ri
import rf_ref
import varimp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FORESTS = {}


def _forest(hip, name):
    """the 20-tree forest of rf_inputs.<name>() with the package's defaults, fitted once"""
    if name not in _FORESTS:
        X, y, inbag, seeds = getattr(ri, name)()
        _FORESTS[name] = (hip.models.RandomForest.fit(X, y, 20, inbag=inbag, seeds=seeds), X, y, inbag)
    return _FORESTS[name]


def _perm_seeds(n_trees, salt):
    return np.random.default_rng([91, salt]).integers(0, 2 ** 64, size=n_trees, dtype=np.uint64)


def _bound(y, inbag):
    R = float(y.max() - y.min())
    return 4.0 * int((np.asarray(inbag) == 0).sum(axis=1).max()) * 2.0 ** -53 * R * R


def _check(m, X, y, inbag, n_perm, what):
    """tree_delta against the restatement on the device's own trees, IncMSE and SD against the formulas on the device's deltas"""
    want = varimp_ref.forest_delta(m.params, X, y, inbag, m.perm_seeds, n_perm)
    bound = _bound(y, inbag)
    err = np.abs(m.tree_delta - want).max()
    print(what, "n_perm", n_perm, "max |delta - restatement|", err, "bound", bound, "max |delta|", np.abs(want).max())
    assert m.tree_delta.shape == want.shape and err <= bound
    inc, sd = varimp_ref.inc_mse(m.tree_delta)
    assert np.allclose(m.importance[:, 0], inc, rtol=1e-12, atol=0) and np.allclose(m.importance_sd, sd, rtol=1e-12, atol=0)
    return want


@pytest.mark.parametrize("name", ["stations", "small"])
@pytest.mark.parametrize("n_perm", [1, 3])
def test_against_the_restatement(hip, name, n_perm):
    m, X, y, inbag = _forest(hip, name)
    seeds = _perm_seeds(20, n_perm)
    imp = m.importance(X, y, perm_seeds=seeds, n_perm=n_perm)
    assert imp.shape == (X.shape[1], 2) and np.array_equal(imp[:, 1], m.inc_node_purity) and np.array_equal(m.perm_seeds, seeds)
    want = _check(m, X, y, inbag, n_perm, name)
    assert np.abs(want).max() > 1e-2                      # (a wrong permutation is off by that much, not by 1e-12)
    if name == "small":                                   # sanity: variable 0 carries the sine term
        print("%IncMSE", imp[:, 0], "SD", m.importance_sd)
        assert np.argmax(imp[:, 0]) == 0


def test_unused_variables_cost_nothing(hip):
    """mtry = 1, nodesize = 400 on the 813 stations: trees of 5 - 15 nodes, each testing 2 - 6 of the 7 variables"""
    X, y, inbag, seeds = ri.stations()
    m = hip.models.RandomForest.fit(X, y, 20, mtry=1, nodesize=400, inbag=inbag, seeds=seeds)
    m.importance(X, y, perm_seeds=_perm_seeds(20, 5), n_perm=2)
    _check(m, X, y, inbag, 2, "unused")
    used = np.stack([varimp_ref.used_variables(rf_ref.tree_of(m.params, t), 7) for t in range(20)])
    print("used (tree, variable) pairs", int(used.sum()), "of", used.size)
    assert used.any() and (~used).any()
    assert np.all(m.tree_delta[~used] == 0.0) and np.any(m.tree_delta[used] != 0.0)


def test_edges(hip):
    models = hip.models
    # a tree without an out-of-bag row between two ordinary ones: a zero row, and the means still divide by n_trees
    X, y, inbag, seeds = ri.small(3)
    inbag = inbag.copy()
    inbag[1] = 1
    m = models.RandomForest.fit(X, y, 3, mtry=2, inbag=inbag, seeds=seeds)
    for n_perm in (1, 3):
        m.importance(X, y, perm_seeds=_perm_seeds(3, 6), n_perm=n_perm)
        _check(m, X, y, inbag, n_perm, "m = 0")
        assert np.all(m.tree_delta[1] == 0.0) and np.any(m.tree_delta[0] != 0.0) and np.any(m.tree_delta[2] != 0.0)
        assert np.array_equal(m.importance[:, 0], (m.tree_delta[0] + m.tree_delta[1] + m.tree_delta[2]) / 3)
    # exactly one out-of-bag row: the permutation is the identity, delta is exactly 0
    inbag[1, 123] = 0
    m = models.RandomForest.fit(X, y, 3, mtry=2, inbag=inbag, seeds=seeds)
    for n_perm in (1, 3):
        m.importance(X, y, perm_seeds=_perm_seeds(3, 7), n_perm=n_perm)
        _check(m, X, y, inbag, n_perm, "m = 1")
        assert np.all(m.tree_delta[1] == 0.0) and np.any(m.tree_delta[0] != 0.0)
    # constant response: root-only trees, no variable is used
    X, _, inbag, seeds = ri.small(5)
    mc = models.RandomForest.fit(X, np.full(300, 2.5), 5, inbag=inbag, seeds=seeds)
    mc.importance(X, np.full(300, 2.5), perm_seeds=_perm_seeds(5, 8), n_perm=2)
    assert not mc.tree_delta.any() and not mc.importance[:, 0].any() and not mc.importance_sd.any()
    # out-of-bag counts that end at, just before and just after a wave's 64 rows, and past two steps
    X, y = ri.plain(200, 3, 60)
    rng = np.random.default_rng(61)
    counts = (63, 64, 65, 129)
    inbag = np.ones((len(counts), 200), dtype=np.int32)
    for t, m_oob in enumerate(counts):
        inbag[t, rng.permutation(200)[:m_oob]] = 0
    m = models.RandomForest.fit(X, y, len(counts), mtry=2, inbag=inbag, seeds=np.arange(4, dtype=np.uint64) + 5)
    assert tuple((inbag == 0).sum(axis=1)) == counts
    for n_perm in (1, 3):
        m.importance(X, y, perm_seeds=_perm_seeds(4, 9), n_perm=n_perm)
        want = _check(m, X, y, inbag, n_perm, "wave edges")
        assert np.all(np.abs(want).max(axis=1) > 0)


def test_beyond_the_on_chip_rows(hip):
    """n just past RI_LDS_ROWS: the row list, the keys and the permutation live in device memory, read by the same code;
    with nodesize 1 the trees also exceed the node records kept on chip.  A small forest in the same call stays on chip."""
    src = open(os.path.join(ROOT, "machisplin_amd", "csrc", "rf_importance.hip")).read()
    limit = int(re.search(r"constexpr int RI_LDS_ROWS = (\d+);", src).group(1))
    nodes = int(re.search(r"constexpr int RI_LDS_NODES = (\d+);", src).group(1))
    n = limit + 200
    X, y = ri.plain(n, 4, 62)
    inbag, seeds = ri.bags_for(n, 3, 63)
    ps = _perm_seeds(3, 10)
    big = {}
    for nodesize in (5, 1):
        m = hip.models.RandomForest.fit(X, y, 3, nodesize=nodesize, inbag=inbag, seeds=seeds)
        m.importance(X, y, perm_seeds=ps)
        _check(m, X, y, inbag, 1, "n = %d, nodesize %d, largest tree %d nodes" % (n, nodesize, np.diff(m.params["tree_offsets"]).max()))
        big[nodesize] = m
    assert np.diff(big[1].params["tree_offsets"]).max() > nodes
    Xs, ys = ri.plain(500, 4, 64)
    bs, ss = ri.bags_for(500, 3, 65)
    small = hip.models.RandomForest.fit(Xs, ys, 3, inbag=bs, seeds=ss)
    alone = small.importance(Xs, ys, perm_seeds=ps).copy()
    alone_delta, big_delta = small.tree_delta.copy(), big[1].tree_delta.copy()
    hip.models.rf_importance_many([big[1], small], [X, Xs], [y, ys], perm_seeds=[ps, ps])
    assert np.array_equal(small.tree_delta, alone_delta) and np.array_equal(small.importance, alone)
    assert np.array_equal(big[1].tree_delta, big_delta)


def test_batches_repeats_and_loaded_forests(hip):
    models = hip.models
    a, Xa, ya, ba = _forest(hip, "small")
    Xb, yb = ri.plain(1500, 5, 66)
    bb, sb = ri.bags_for(1500, 20, 67)
    b = models.RandomForest.fit(Xb, yb, 20, inbag=bb, seeds=sb)
    pa, pb = _perm_seeds(20, 11), _perm_seeds(20, 12)
    one_a = (a.importance(Xa, ya, perm_seeds=pa, n_perm=2).copy(), a.importance_sd.copy(), a.tree_delta.copy())
    one_b = (b.importance(Xb, yb, perm_seeds=pb, n_perm=2).copy(), b.importance_sd.copy(), b.tree_delta.copy())
    # two forests of different n in one call: the single calls bit for bit; and the same call twice
    for _ in range(2):
        models.rf_importance_many([b, a], [Xb, Xa], [yb, ya], perm_seeds=[pb, pa], n_perm=2)
        for m, one in ((a, one_a), (b, one_b)):
            assert np.array_equal(m.importance, one[0]) and np.array_equal(m.importance_sd, one[1]) and np.array_equal(m.tree_delta, one[2])
    # a forest loaded from the same arrays: the same numbers (its inbag has to be given; IncNodePurity is unknown)
    loaded = models.from_param_dict(a.params)
    with pytest.raises(ValueError):
        loaded.importance(Xa, ya, perm_seeds=pa, n_perm=2)
    imp = loaded.importance(Xa, ya, inbag=ba, perm_seeds=pa, n_perm=2)
    assert np.array_equal(imp[:, 0], one_a[0][:, 0]) and np.all(np.isnan(imp[:, 1])) and np.array_equal(loaded.tree_delta, one_a[2])
    # other seeds, other permutations
    assert not np.array_equal(a.importance(Xa, ya, perm_seeds=pb, n_perm=2)[:, 0], one_a[0][:, 0])


def test_fit_with_importance_and_default_seeds(hip):
    """importance = True runs the call after the fit: the forest, its bags and its draw seeds are those of the plain fit,
    and the permutation seeds come from a stream of their own"""
    models = hip.models
    X, y, _, _ = ri.small(1)
    plain = models.RandomForest.fit(X, y, 20, seed=5)
    m = models.RandomForest.fit(X, y, 20, seed=5, importance=True, n_perm=2)
    assert np.array_equal(m.inbag, plain.inbag) and np.array_equal(m.seeds, plain.seeds)
    assert all(np.array_equal(m.params[k], plain.params[k]) for k in ("tree_offsets",) + rf_ref.KEYS)
    assert np.array_equal(m.perm_seeds, np.random.default_rng([5, 2 ** 20]).integers(0, 2 ** 64, size=20, dtype=np.uint64))
    _check(m, X, y, m.inbag, 2, "importance = True")
    assert np.array_equal(plain.importance(X, y, n_perm=2, seed=5), m.importance)
    assert np.argmax(m.importance[:, 0]) == 0
    # two forests in one fit call: model k's permutation seeds from [seed, k, 2^20]
    two = models.rf_fit_many([X, X[:200]], [y, y[:200]], 5, seed=5, importance=True)
    assert np.array_equal(two[1].perm_seeds, np.random.default_rng([5, 1, 2 ** 20]).integers(0, 2 ** 64, size=5, dtype=np.uint64))
    assert np.array_equal(two[1].inbag, models.rf_fit_many([X, X[:200]], [y, y[:200]], 5, seed=5)[1].inbag)


def test_errors(hip):
    from machisplin_amd import _lib
    models = hip.models
    m, X, y, inbag = _forest(hip, "small")
    ps = _perm_seeds(20, 13)

    def refused(model=m, X=X, y=y, inbag=inbag, n_perm=1):
        with pytest.raises(hip.MhsError) as ei:
            models.rf_importance_many([model], [X], [y], [inbag], [ps], n_perm)
        assert ei.value.code == _lib.ERR_INVALID

    refused(n_perm=0)
    refused(n_perm=17)
    Xn = X.copy()
    Xn[17, 2] = np.nan
    refused(X=Xn)
    yi = y.copy()
    yi[5] = -np.inf
    refused(y=yi)
    neg = inbag.copy()
    neg[3, 5] = -1
    refused(inbag=neg)
    refused(X=np.column_stack([X, X[:, 0]]))                        # the forest has p = 5
    # a handle that is no forest, and NULL arguments, through the C ABI
    lib = _lib.lib()
    Xf = np.asfortranarray(X)
    pa = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    ns = np.array([300], dtype=np.int64)
    out = np.empty(5)
    gam = models.Gam.fit(X, y)
    call = lambda h, Xp, bp: lib.mhs_rf_importance_many(1, h, Xp, pa(y), ns.ctypes.data, 5, bp, pa(ps), 1, pa(out), None, None)
    assert call((C.c_void_p * 1)(gam._h), pa(Xf), pa(inbag)) == _lib.ERR_INVALID
    assert call((C.c_void_p * 1)(None), pa(Xf), pa(inbag)) == _lib.ERR_INVALID
    assert call((C.c_void_p * 1)(m._h), None, pa(inbag)) == _lib.ERR_INVALID
    assert call((C.c_void_p * 1)(m._h), pa(Xf), (C.c_void_p * 1)(None)) == _lib.ERR_INVALID
    assert call((C.c_void_p * 1)(m._h), pa(Xf), pa(inbag)) == _lib.OK       # ... and with nothing wrong it runs; two outputs NULL
    assert np.array_equal(out, m.importance(X, y, perm_seeds=ps)[:, 0])
