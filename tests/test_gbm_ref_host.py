"""CPU: the numpy reference of the gbm growth rule (tests/gbm_ref.py) against an independent implementation, and the
condition that makes an exact structural comparison with the device fair -- on every input test_gbm_fit_gpu.py compares
structurally, accumulating the left sums in float64 and in extended precision gives identical trees."""
import numpy as np
import pytest

import gbm_inputs as gi
import gbm_ref


def test_reference_agrees_with_scikit_learn():
    """Every row in every bag: best-first growth to 26 leaves with >= 10 rows per leaf is what scikit-learn's regressor
    does with max_leaf_nodes = 26 (8 trees, learning rate 0.1)."""
    import sklearn.ensemble as ske
    X, y, _ = gi.short()
    n = y.size
    bags = [np.arange(n)] * 8
    params, F, trees = gbm_ref.fit(X, y, 8, bags, depth=25, minobs=10, shrinkage=0.1)
    g = ske.GradientBoostingRegressor(n_estimators=8, learning_rate=0.1, max_leaf_nodes=26, max_depth=None, min_samples_leaf=10,
                                      subsample=1.0, criterion="squared_error").fit(X, y)
    assert np.abs(F - g.predict(X)).max() < 1e-12
    ours = [int(np.sum(t["split_var"] < 0) - np.sum(t["split_var"] >= 0)) for t in trees]      # leaves without the missing nodes
    assert ours == [int(e[0].tree_.n_leaves) for e in g.estimators_]


def _chain_stable(X, y, bags, compared, shrinkage=0.01):
    """Grow the float64 chain; at every tree in ``compared`` (1-based) also grow the extended-precision tree from the
    same F.  Returns the number of compared trees whose structures differ."""
    orders = gbm_ref.sort_orders(X)
    F = np.full(y.size, float(np.mean(y)))
    bad = 0
    for t in range(1, max(compared) + 1):
        z = y - F
        tr = gbm_ref.grow_tree(X, z, bags[t - 1], orders, 25, 10, shrinkage)
        if t in compared:
            bad += not gbm_ref.same_structure(tr, gbm_ref.grow_tree(X, z, bags[t - 1], orders, 25, 10, shrinkage, acc=np.longdouble))
        F = F + gbm_ref.tree_values(tr, X)
    return bad


@pytest.mark.parametrize("name", ["short", "stations"])
def test_short_inputs_do_not_hinge_on_the_summation_order(name):
    X, y, bags = getattr(gi, name)()
    a = gbm_ref.fit(X, y, 40, bags)[2]
    b = gbm_ref.fit(X, y, 40, bags, acc=np.longdouble)[2]
    assert all(gbm_ref.same_structure(s, t) for s, t in zip(a, b))


def test_long_input_does_not_hinge_on_the_summation_order():
    """the teacher-forced comparison's trees (every 25th of 500, ten models): no tree that float64 and extended
    precision order differently, so the near-tie allowance of the GPU test is not needed by the reference itself"""
    for X, y, bags in gi.long_models():
        assert _chain_stable(X, y, bags, set(range(gi.LONG_EVERY, bags.shape[0] + 1, gi.LONG_EVERY))) == 0


def test_large_input_does_not_hinge_on_the_summation_order():
    X, y, bags = gi.large()
    assert _chain_stable(X, y, bags, set(gi.LARGE_SAMPLED)) == 0


def test_reference_invariants():
    X, y, bags = gi.short()
    params, F, trees = gbm_ref.fit(X, y, 5, bags)
    from oracle import ensemble as oe
    assert np.abs(oe.predict(params, X) - F).max() < 1e-13
    for t in trees:
        assert np.sum(t["split_var"] >= 0) <= 25
        assert t["split_var"].size == 3 * np.sum(t["split_var"] >= 0) + 1
