"""CPU: the host rules of machisplin_amd/varimp.py on hand-made inputs, and the restatement of the forest's permutations
(tests/varimp_ref.py) that the GPU tests compare the device with."""
import numpy as np

import rf_ref
import varimp_ref
from machisplin_amd import varimp


def test_garson_hand_computed():
    """p = 2, size = 2.  Hidden 1: w = (1, -3), v = 2 -> Q = (2, 6), r = (1/4, 3/4); hidden 2: w = (-2, 2), v = -0.5 ->
    Q = (1, 1), r = (1/2, 1/2); rel_imp = (3/4, 5/4) / 2.  The biases (9, -7, 5) play no part."""
    wts = np.array([9.0, 1.0, -3.0, -7.0, -2.0, 2.0, 5.0, 2.0, -0.5])
    g = varimp.garson(wts, 2, 2)
    assert np.allclose(g, [0.375, 0.625], rtol=1e-15, atol=0)
    assert abs(g.sum() - 1.0) <= 1e-15
    other = wts.copy()
    other[[0, 3, 6]] = [-1.0, 0.0, 100.0]
    assert np.array_equal(varimp.garson(other, 2, 2), g)
    rng = np.random.default_rng(0)
    w = rng.normal(size=(5 + 1) * 10 + 11)
    assert np.allclose(varimp.garson(w, 5, 10), varimp_ref.garson(w, 5, 10), rtol=1e-13, atol=0)
    assert abs(varimp.garson(w, 5, 10).sum() - 1.0) <= 1e-14


def test_evimp_hand_built_record():
    """Four forward terms over p = 3: the intercept, a hinge pair on variable 1, a linear term on variable 0; three are
    selected.  Size 2 keeps {0, 1} (variable 1), size 3 keeps {0, 1, 3} (variables 1 and 0); variable 2 is never used."""
    fdirs = np.array([[0, 0, 0], [0, 1, 0], [0, -1, 0], [2, 0, 0]], dtype=np.int32)
    pt = np.array([[0, -1, -1, -1], [0, 1, -1, -1], [0, 1, 3, -1], [0, 1, 2, 3]], dtype=np.int32)
    rec = {"forward": {"dirs": fdirs}, "prune_terms": pt, "selected": np.array([True, True, False, True]),
           "gcv_per_subset": np.array([10.0, 6.0, 5.0, 5.5]), "rss_per_subset": np.array([100.0, 36.0, 20.0, 19.0])}
    nsub, gcv, rss, order = varimp.evimp(rec, 3)
    assert np.array_equal(nsub, [1, 2, 0])
    # variable 1: gcv (10 - 6) + (6 - 5) = 5, rss 64 + 16 = 80; variable 0: gcv 1, rss 16; then sqrt, the largest = 100
    assert np.allclose(gcv, [100.0 * np.sqrt(1.0 / 5.0), 100.0, 0.0], rtol=1e-14, atol=0)
    assert np.allclose(rss, [100.0 * np.sqrt(16.0 / 80.0), 100.0, 0.0], rtol=1e-14, atol=0)
    assert np.array_equal(order, [1, 0, 2])
    # a subset whose GCV rises takes its (negative) difference off the variables it uses
    rec2 = dict(rec, selected=np.array([True, True, True, True]))
    _, gcv2, _, _ = varimp.evimp(rec2, 3)
    assert np.allclose(gcv2, [100.0 * np.sqrt(0.5 / 4.5), 100.0, 0.0], rtol=1e-14, atol=0)      # variable 0: 1 - 0.5, variable 1: 5 - 0.5
    # only the intercept selected: nothing to rank
    nsub0, gcv0, rss0, order0 = varimp.evimp(dict(rec, selected=np.array([True, False, False, False])), 3)
    assert not nsub0.any() and not gcv0.any() and not rss0.any() and np.array_equal(order0, [0, 1, 2])


def test_breakdown_up_on_a_linear_predict():
    """f(x) = a + beta . x: whatever the greedy order, c_v = beta_v (x*_v - mean D_v), and the contributions add up to
    f(x*) - mean f(D)"""
    rng = np.random.default_rng(1)
    D = rng.normal(size=(40, 4)) + np.array([0.0, 3.0, -1.0, 2.0])
    beta = np.array([1.5, -0.2, 0.0, 3.0])
    f = lambda Z: 0.7 + Z @ beta
    xs = rng.normal(size=(6, 4))
    want = beta * (xs - D.mean(axis=0))
    scale = np.abs(f(D)).max()
    for x, w in zip(xs, want):
        c, b0 = varimp.breakdown_up(f, x, D)
        assert np.abs(c - w).max() <= 1e-13 * scale and abs(b0 - f(D).mean()) <= 1e-13 * scale
        assert abs(c.sum() - (f(x[None, :])[0] - b0)) <= 1e-13 * scale
        c_ref, b_ref = varimp_ref.breakdown_up(f, x, D)
        assert np.abs(c - c_ref).max() <= 1e-13 * scale and abs(b0 - b_ref) <= 1e-13 * scale
    C, b0 = varimp.breakdown_up_many(f, xs, D)
    assert np.abs(C - want).max() <= 1e-13 * scale
    # an interaction makes the order matter: the batched greedy choice is the restatement's, observation by observation
    g = lambda Z: np.sin(Z[:, 0]) * Z[:, 1] + 0.5 * Z[:, 2] * Z[:, 3]
    C, b0 = varimp.breakdown_up_many(g, xs, D)
    for x, c in zip(xs, C):
        c_ref, b_ref = varimp_ref.breakdown_up(g, x, D)
        assert np.abs(c - c_ref).max() <= 1e-13 * np.abs(g(D)).max() and abs(b0 - b_ref) <= 1e-13
    # ksvm_contributions: mean |c| over the sample rows, the sample drawn without replacement from its own stream
    class Lin:
        predict_points = staticmethod(f)
    got = varimp.ksvm_contributions(Lin, D, sample=10, seed=3)
    rows = np.random.default_rng(3).choice(40, 10, replace=False)
    S = D[rows]
    assert np.abs(got - np.mean(np.abs(beta * (S - S.mean(axis=0))), axis=0)).max() <= 1e-13 * scale
    assert np.array_equal(varimp.ksvm_contributions(Lin, D, rows=rows), got)
    assert got[2] == 0.0


def test_the_restated_permutation():
    p, m = 7, 300
    seen = set()
    for k in range(3):
        for v in range(p):
            s = varimp_ref.permutation(0x1234567890ABCDEF, k, v, p, m)
            assert np.array_equal(np.sort(s), np.arange(m))
            assert not np.array_equal(s, np.arange(m))
            seen.add(s.tobytes())
    assert len(seen) == 3 * p                                                   # changes with k and with v
    assert not np.array_equal(varimp_ref.permutation(1, 0, 0, p, m), varimp_ref.permutation(2, 0, 0, p, m))
    # h = mix(s + k p + v): (k, v) and (k - 1, v + p) would share a stream, v < p keeps them apart; m = 1 and 0 are trivial
    assert np.array_equal(varimp_ref.permutation(5, 1, 0, p, m), varimp_ref.permutation(5, 0, p, p, m))
    assert np.array_equal(varimp_ref.permutation(5, 0, 0, p, 1), [0]) and varimp_ref.permutation(5, 0, 0, p, 0).size == 0


def test_the_restated_importance_sees_the_signal():
    """a CPU forest on rf_inputs.small: permuting variable 0 (the sine term) costs the most; an unused variable costs 0"""
    import rf_inputs as ri
    X, y, inbag, seeds = ri.small(6)
    trees = [rf_ref.grow_tree(X, y, inbag[t], seeds[t], 2, 5) for t in range(6)]
    perm_seeds = np.arange(6, dtype=np.uint64) + 77
    delta = np.stack([varimp_ref.tree_delta(tr, X, y, inbag[t], perm_seeds[t], 1) for t, tr in enumerate(trees)])
    inc, sd = varimp_ref.inc_mse(delta)
    assert np.argmax(inc) == 0 and inc[0] > 0.3 and np.all(sd >= 0)
    stump = {k: np.asarray(v) for k, v in dict(left=[2, 0, 0], right=[3, 0, 0], status=[-3, -1, -1], best_var=[2, 0, 0], split=[0.0, 0.0, 0.0],
                                               node_pred=[0.0, -1.0, 1.0]).items()}
    d = varimp_ref.tree_delta(stump, X, y, inbag[0], 9, 2)
    assert np.array_equal(d != 0.0, [False, True, False, False, False])
