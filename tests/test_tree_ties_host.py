"""CPU: what makes the exact comparisons of test_tree_ties_gpu.py fair, and what gives them teeth.

Fair: on the inputs of exact_inputs.py every partial sum is an integer below 2^53, so the references grow the same trees
-- every array bit for bit -- whether they add sequentially (np.cumsum) or in the device's order (64-row steps, a
log-depth scan inside the step).  (float64 against np.longdouble is NOT compared: the criterion's own rounding differs
between the two formats even with exact sums, and the device is float64.)

Teeth: the references take three DELIBERATELY WRONG tie-breaks as keyword arguments -- (a) cross-variable ties to the last
variable ('>=' in the combine), (b) within-variable ties to the highest position, (c) gbm only: the terminal-list tie to
the later node.  Per case of the GPU module the trees each variant changes are counted and printed, and a case is
admitted only if (a) changes at least one tree in four (not asked of the forest at mtry 1, where a node has one
variable), (b) changes at least one tree, and (c) changes at least one tree in at least one gbm case: a kernel with one
of those mistakes could not pass the GPU module."""
import numpy as np
import pytest

import exact_inputs as xi
import gbm_ref
import rf_ref

RF_ARRAYS = rf_ref.KEYS
GBM_ARRAYS = ("split_var", "split_val", "left", "right", "missing", "imp")


def _same(a, b, keys):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _rf_trees(case, **kw):
    X, y, inbag, seeds, mtry, nodesize = case
    return [rf_ref.grow_tree(X, y, inbag[t], seeds[t], mtry, nodesize, **kw) for t in range(inbag.shape[0])]


def _gbm_trees(X, z, bags, depth, minobs, **kw):
    orders = gbm_ref.sort_orders(X)
    return [gbm_ref.grow_tree(X, z, b, orders, depth, minobs, **kw) for b in bags]


def _rf_tie_nodes(case, trees):
    """(internal nodes whose best criterion is reached by more than one drawn variable, ... by more than one position of
    the first variable that reaches it), bit-equal criteria only"""
    X, y, inbag, seeds, mtry, _ = case
    cross = within = 0
    for t, tr in enumerate(trees):
        counts = np.asarray(inbag[t], dtype=np.int64)
        for k in np.flatnonzero(tr["status"] == -3):
            crits = [rf_ref._candidates(X, y, counts, tr["rows"][k], v, np.float64)[0] for v in rf_ref.draw_vars(seeds[t], k, X.shape[1], mtry)]
            tops = [c.max() for c in crits if c.size]
            best = max(tops)
            cross += sum(1 for m in tops if m == best) > 1
            within += int(np.sum(next(c for c in crits if c.size and c.max() == best) == best)) > 1
    return cross, within


def _gbm_tie_nodes(X, z, trees, minobs):
    """the same two counts over the internal nodes of gbm's trees (variables in index order)"""
    cross = within = 0
    for tr in trees:
        for e, o in tr["pre"].items():
            if tr["split_var"][o] < 0:
                continue
            imps = [gbm_ref._improvements(X[r, v], np.cumsum(z[r]), tr["tot"][e], r.size, minobs)[0] for v, r in enumerate(tr["segs"][e])]
            best = max(i.max() for i in imps)
            cross += sum(1 for i in imps if i.max() == best) > 1
            within += int(np.sum(next(i for i in imps if i.max() == best) == best)) > 1
    return cross, within


def _changed(a, b, keys):
    return sum(not _same(s, t, keys) for s, t in zip(a, b))


def test_assert_exact_refuses_what_is_not_exact():
    xi.assert_exact(np.array([3.0, -2.0, 0.0]), np.array([0, 4, 1]))
    with pytest.raises(AssertionError):
        xi.assert_exact(np.array([3.0, 0.5]))
    with pytest.raises(AssertionError):
        xi.assert_exact(np.array([3.0, np.nan]))
    with pytest.raises(AssertionError):
        xi.assert_exact(np.array([2.0 ** 40, 1.0]), np.full(2, 2 ** 13))
    with pytest.raises(AssertionError):
        xi.assert_exact(np.array([1.0, 2.0]), np.array([1.5, 1.0]))


def test_device_scan_is_the_sequential_sum_on_integers_and_not_on_fractions():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 129, 1000):
        a = rng.integers(-500, 500, size=n).astype(np.float64)
        assert np.array_equal(xi.device_scan(a), np.cumsum(a))
    b = rng.normal(size=1000)
    assert np.allclose(xi.device_scan(b), np.cumsum(b), rtol=0, atol=1e-12) and not np.array_equal(xi.device_scan(b), np.cumsum(b))


@pytest.mark.parametrize("name", sorted(xi.RF_CASES))
def test_forest_case(name):
    """the reference's trees do not depend on the order of addition, and the wrong tie-breaks change them"""
    case = xi.rf_case(name)
    mtry, n_trees = case[4], case[2].shape[0]
    seq = _rf_trees(case)
    assert all(_same(s, t, RF_ARRAYS) for s, t in zip(seq, _rf_trees(case, scan=xi.device_scan)))
    a = _changed(seq, _rf_trees(case, var_tie_last=True), RF_ARRAYS)
    b = _changed(seq, _rf_trees(case, pos_tie_high=True), RF_ARRAYS)
    internal = sum(int(np.sum(t["status"] == -3)) for t in seq)
    cross, within = _rf_tie_nodes(case, seq)
    print("forest %-16s n %5d trees %2d internal nodes %5d, exact ties across variables %4d, within the variable %3d; "
          "trees changed by (a) last variable %d, (b) highest position %d" % (name, case[1].size, n_trees, internal, cross, within, a, b))
    assert mtry == 1 or 4 * a >= n_trees
    assert b >= 1


def _gbm_case_counts(label, X, z, bags, depth, minobs):
    seq = _gbm_trees(X, z, bags, depth, minobs)
    assert all(_same(s, t, GBM_ARRAYS) for s, t in zip(seq, _gbm_trees(X, z, bags, depth, minobs, scan=xi.device_scan)))
    a = _changed(seq, _gbm_trees(X, z, bags, depth, minobs, var_tie_last=True), GBM_ARRAYS)
    b = _changed(seq, _gbm_trees(X, z, bags, depth, minobs, pos_tie_high=True), GBM_ARRAYS)
    c = _changed(seq, _gbm_trees(X, z, bags, depth, minobs, node_tie_later=True), GBM_ARRAYS)
    internal = sum(int(np.sum(t["split_var"] >= 0)) for t in seq)
    cross, within = _gbm_tie_nodes(X, z, seq, minobs)
    print("gbm %-16s n %5d trees %2d internal nodes %5d, exact ties across variables %4d, within the variable %3d; "
          "trees changed by (a) last variable %d, (b) highest position %d, (c) later node %d"
          % (label, z.size, len(bags), internal, cross, within, a, b, c))
    assert 4 * a >= len(bags)
    assert b >= 1
    return c


_later_node = {}


@pytest.mark.parametrize("name", sorted(xi.GBM_CASES))
def test_gbm_first_tree_case(name):
    X, y, bags, depth, minobs = xi.gbm_case(name)
    _later_node[name] = _gbm_case_counts(name, X, y - y.sum() / y.size, bags, depth, minobs)


@pytest.mark.parametrize("name", sorted(xi.GBM_LATER))
def test_gbm_later_tree_case(name):
    X, y, F, bags, depth, minobs = xi.gbm_later_case(name)
    _later_node["later-" + name] = _gbm_case_counts("later-" + name, X, y - F, bags, depth, minobs)


def test_gbm_some_case_hinges_on_the_terminal_list_order():
    """(c): in at least one gbm case the later-node variant changes a tree (after the cases above it sees all their
    counts; alone it counts the case made for this)"""
    if "tied-depth64" not in _later_node:
        test_gbm_first_tree_case("tied-depth64")
    print("trees changed by (c) per case:", _later_node)
    assert max(_later_node.values()) >= 1
