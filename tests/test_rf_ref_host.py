"""CPU: the numpy reference of the random-forest growth rule (tests/rf_ref.py) against an independent implementation,
its certificate walk against its own trees and against mutated ones, and the counter-based variable draw."""
import numpy as np
import pytest

import rf_inputs as ri
import rf_ref


@pytest.mark.parametrize("name", ["small", "stations"])
def test_reference_agrees_with_scikit_learn(name):
    """mtry = p, nodesize 5: a node is split when its population is >= 6, which is scikit-learn's tree with
    min_samples_split = 6 on the bag with its rows DUPLICATED.  Equal node counts, in-bag predictions equal to
    1e-12 max|y|, on 10 bags.  (The structures need not be equal: two variables that cut off the same rows tie.)"""
    from sklearn.tree import DecisionTreeRegressor
    X, y, inbag, seeds = getattr(ri, name)(10)
    p = X.shape[1]
    for t in range(10):
        tr = rf_ref.grow_tree(X, y, inbag[t], seeds[t], p, 5)
        dup = np.repeat(np.arange(y.size), inbag[t])
        sk = DecisionTreeRegressor(min_samples_split=6, random_state=0).fit(X[dup], y[dup])
        assert sk.tree_.node_count == tr["left"].size
        rows = np.flatnonzero(inbag[t] > 0)
        assert np.abs(sk.predict(X[rows]) - rf_ref.predict(tr, X[rows])).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("acc", [np.float64, np.longdouble])
@pytest.mark.parametrize("name,mtry,nodesize", [("small", 1, 5), ("small", 5, 1), ("stations", 2, 5), ("stations", 7, 40)])
def test_the_certificate_accepts_the_reference(name, mtry, nodesize, acc):
    """check_tree (float64 criteria) accepts the reference's own trees grown with either accumulator"""
    X, y, inbag, seeds = getattr(ri, name)(4)
    for t in range(4):
        tr = rf_ref.grow_tree(X, y, inbag[t], seeds[t], mtry, nodesize, acc=acc)
        res = rf_ref.check_tree(X, y, inbag[t], seeds[t], mtry, nodesize, tr)
        assert res["nodes"] == tr["left"].size
        rows = np.flatnonzero(inbag[t] > 0)
        assert np.array_equal(res["leaf"][rows], rf_ref.terminal_nodes(tr, X[rows]))


def _copy(tr):
    return {k: np.array(tr[k]) for k in rf_ref.KEYS}


def test_the_certificate_rejects_mutations():
    X, y, inbag, seeds = ri.stations(1)
    p = X.shape[1]
    # one split moved to the next candidate (the root, all variables drawn)
    tr = rf_ref.grow_tree(X, y, inbag[0], seeds[0], p, 5)
    rf_ref.check_tree(X, y, inbag[0], seeds[0], p, 5, tr)
    bad = _copy(tr)
    v = int(bad["best_var"][0]) - 1
    xs = np.unique(X[inbag[0] > 0, v])
    at = int(np.searchsorted(xs, bad["split"][0], side="right"))        # xs[at - 1] <= split < xs[at]
    bad["split"][0] = rf_ref.split_value(xs[at], xs[at + 1])
    with pytest.raises(AssertionError):
        rf_ref.check_tree(X, y, inbag[0], seeds[0], p, 5, bad)
    # one variable outside the draw
    tr = rf_ref.grow_tree(X, y, inbag[0], seeds[0], 2, 5)
    rf_ref.check_tree(X, y, inbag[0], seeds[0], 2, 5, tr)
    bad = _copy(tr)
    k = int(np.flatnonzero(bad["status"] == -3)[3])
    drawn = rf_ref.draw_vars(seeds[0], k, p, 2)
    bad["best_var"][k] = 1 + next(u for u in range(p) if u not in drawn)
    with pytest.raises(AssertionError, match="not among the drawn"):
        rf_ref.check_tree(X, y, inbag[0], seeds[0], 2, 5, bad)
    # one wrong node_pred
    bad = _copy(tr)
    bad["node_pred"][7] += 1e-6
    with pytest.raises(AssertionError, match="node_pred"):
        rf_ref.check_tree(X, y, inbag[0], seeds[0], 2, 5, bad)
    # a node split although its population is <= nodesize is caught through the numbering / population rules
    with pytest.raises(AssertionError):
        rf_ref.check_tree(X, y, inbag[0], seeds[0], 2, 40, tr)


def test_the_draw():
    """mtry distinct variables; over 20 000 nodes at p = 7, mtry = 2 every variable is drawn between 0.9 and 1.1 times
    its expected count (20 000 * 2 / 7 = 5 714)"""
    hits = np.zeros(7, dtype=np.int64)
    for k in range(20000):
        d = rf_ref.draw_vars(0x1234567890ABCDEF, k, 7, 2)
        assert len(set(d)) == 2 and all(0 <= u < 7 for u in d)
        hits[d] += 1
    print("draws per variable", hits)
    assert np.all(hits >= 0.9 * 40000 / 7) and np.all(hits <= 1.1 * 40000 / 7)
    for p, mtry in ((5, 5), (64, 21), (2, 1)):
        d = rf_ref.draw_vars(2 ** 64 - 1, 3, p, mtry)
        assert len(set(d)) == mtry and all(0 <= u < p for u in d)
    assert sorted(rf_ref.draw_vars(7, 0, 5, 5)) == [0, 1, 2, 3, 4]
