"""GPU: the tie-break rules of the tree fits (rf_fit.hip, gbm_fit.hip; stated in include/machisplin_hip.h), pinned on
inputs whose sums are exact.  Within a variable the lowest position wins among equal criteria; across variables the first
(the forest: in draw order, gbm: in index order); only a strictly greater candidate replaces the best; gbm splits the
terminal node with the strictly greatest improvement in terminal-list order.

On the inputs of exact_inputs.py every partial sum is an integer below 2^53 and the criterion is the same operations in
the same order on the device and in the float64 references (rf_ref.py, gbm_ref.py), so the device must reproduce the
reference BIT FOR BIT: every equality here is np.array_equal.  The only tolerance is the project's 1e-12 max|y| on gbm's
terminal values and on oob_pred.  test_tree_ties_host.py shows per case that the reference does not depend on the order
of addition and that each wrong tie-break would change its trees."""
import ctypes as C
import functools

import numpy as np
import pytest

import earth_inputs as ei
import earth_ref
import exact_inputs as xi
import gbm_ref
import rf_ref

RF_KEYS = ("tree_offsets",) + rf_ref.KEYS
GBM_INT = ("tree_offsets", "split_var", "left", "right", "missing")


# ---------------------------------------------------------------- the forest

@functools.lru_cache(maxsize=None)
def _rf_reference(name):
    """(the case, the reference's trees, their bundle): computed once, shared, never changed"""
    case = xi.rf_case(name)
    X, y, inbag, seeds, mtry, nodesize = case
    xi.assert_exact(y, inbag)
    trees = [rf_ref.grow_tree(X, y, inbag[t], seeds[t], mtry, nodesize, acc=np.float64) for t in range(inbag.shape[0])]
    return case, trees, rf_ref.bundle(trees, X.shape[1])


def _rf_check(name, model):
    (X, y, inbag, _, _, _), trees, want = _rf_reference(name)
    got = model.params
    diff = [k for k in RF_KEYS if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]
    internal = int(np.sum(want["status"] == -3))
    print(name, "n", y.size, "trees", len(trees), "internal nodes", internal, "arrays that differ", diff)
    if diff:
        dev = [rf_ref.tree_of(got, t) for t in range(len(got["tree_offsets"]) - 1)]
        print("trees that differ", [t for t, (a, b) in enumerate(zip(dev, trees)) if any(not np.array_equal(a[k], b[k]) for k in rf_ref.KEYS)])
    assert not diff
    pred, cnt = rf_ref.oob(trees, X, inbag)
    assert np.array_equal(model.oob_count, cnt)
    seen = cnt > 0
    assert np.all(np.isnan(model.oob_pred[~seen]))
    if seen.any():
        assert np.abs(model.oob_pred[seen] - pred[seen]).max() <= 1e-12 * np.abs(y).max()


def _rf_fit(hip, name):
    (X, y, inbag, seeds, mtry, nodesize), _, _ = _rf_reference(name)
    return hip.models.RandomForest.fit(X, y, inbag.shape[0], mtry=mtry, nodesize=nodesize, inbag=inbag, seeds=seeds)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real-mtry1-ns5", "real-mtry2-ns5", "real-mtry4-ns1", "tied-300"])
def test_forest_bit_equal(hip, name):
    """the station table at (mtry, nodesize) = (1, 5), (2, 5), (4, 1) and the rounded table at mtry = p, 10 trees"""
    _rf_check(name, _rf_fit(hip, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", xi.RF_EDGES)
def test_forest_bit_equal_wave_edges(hip, name):
    """n = 63, 64, 65, 129: a segment that ends before, at and after a 64-row step of the prefix scan; every row once,
    nodesize 1"""
    (_, _, inbag, _, _, nodesize), _, _ = _rf_reference(name)
    assert np.all(inbag == 1) and nodesize == 1
    _rf_check(name, _rf_fit(hip, name))


@pytest.mark.gpu
def test_forest_bit_equal_past_the_on_chip_rows(hip):
    """n just past RF_LDS_ROWS: y, the counts and the marks come from device memory"""
    (_, y, _, _, _, _), _, _ = _rf_reference("past-lds")
    limit = xi.rf_lds_rows()
    assert limit == 8192 and limit < y.size <= limit + 64
    _rf_check("past-lds", _rf_fit(hip, "past-lds"))


@pytest.mark.gpu
def test_forest_bit_equal_in_a_batch(hip):
    """two models of different n in one rf_fit_many call: each is bit-equal to its solo reference"""
    names = ("tied-300", "tied-200")
    cases = [_rf_reference(k)[0] for k in names]
    assert cases[0][1].size != cases[1][1].size and cases[0][4:] == cases[1][4:]
    models = hip.models.rf_fit_many([c[0] for c in cases], [c[1] for c in cases], cases[0][2].shape[0], mtry=cases[0][4],
                                    nodesize=cases[0][5], inbag=[c[2] for c in cases], seeds=[c[3] for c in cases])
    for name, m in zip(names, models):
        _rf_check(name, m)


# ---------------------------------------------------------------- gbm

def _gbm_reference_trees(X, z, bags, depth, minobs):
    xi.assert_exact(z)
    orders = gbm_ref.sort_orders(X)
    return [gbm_ref.grow_tree(X, z, b, orders, depth, minobs, 0.01, acc=np.float64) for b in bags]


@functools.lru_cache(maxsize=None)
def _gbm_first_reference(name):
    X, y, bags, depth, minobs = xi.gbm_case(name)
    mean = y.sum() / y.size
    assert mean == np.rint(mean)
    return (X, y, bags, depth, minobs), float(mean), _gbm_reference_trees(X, y - mean, bags, depth, minobs)


def _gbm_check(label, y, devs, refs):
    """every device tree (a dict of its preorder arrays with tree_offsets) against the reference's tree"""
    tol = 1e-12 * np.abs(y).max()
    exact_values = 0
    for t, (dev, ref) in enumerate(zip(devs, refs)):
        nn = ref["split_var"].size
        assert np.array_equal(dev["tree_offsets"], [0, nn]), (label, t, dev["tree_offsets"], nn)
        for k in GBM_INT[1:]:
            assert np.array_equal(dev[k], ref[k]), (label, "tree", t, k, dev[k], ref[k])
        internal = ref["split_var"] >= 0
        assert np.array_equal(dev["split_val"][internal], ref["split_val"][internal]), (label, "tree", t, "split values")
        assert np.abs(dev["split_val"][~internal] - ref["split_val"][~internal]).max() <= tol
        exact_values += bool(np.array_equal(dev["split_val"], ref["split_val"]))
    print(label, "trees", len(refs), "internal nodes", sum(int(np.sum(r["split_var"] >= 0)) for r in refs),
          "trees whose terminal values are bit-equal too:", exact_values)


def _gbm_first(hip, name):
    (X, y, bags, depth, minobs), mean, refs = _gbm_first_reference(name)
    models = hip.models.gbm_fit_many([X] * len(bags), [y] * len(bags), 1, bags=[b[None, :] for b in bags], interaction_depth=depth,
                                     n_minobsinnode=minobs)
    assert all(m.init_f == mean for m in models)
    _gbm_check(name, y, [m.params for m in models], refs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in sorted(xi.GBM_CASES) if k != "large-n"])
def test_gbm_first_trees_bit_equal(hip, name):
    """40 bags of n / 2, every one the first tree of a model of its own (z = y - the integer mean), in one call"""
    _gbm_first(hip, name)


@pytest.mark.gpu
def test_gbm_first_tree_bit_equal_large_n(hip):
    """n = 20 000: z and the flags come from device memory; one model, one tree at the kernel's largest depth"""
    (X, _, bags, depth, _), _, _ = _gbm_first_reference("large-n")
    assert X.shape[0] == xi.GBM_LARGE_N and len(bags) == 1 and depth == 64
    _gbm_first(hip, "large-n")


def _grow_from(X, y, F, bags, depth, minobs, shrinkage=0.01):
    """mhs_gbm_grow_many with first_call = 0: one model per bag, one tree each, all from the caller's F.  Returns per
    model (the tree's arrays, F after the tree)."""
    from machisplin_amd import _lib
    Xf, y = np.asfortranarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    bags = np.ascontiguousarray(bags, dtype=np.int32)
    n, p = Xf.shape
    count, cap = bags.shape[0], 3 * depth + 1
    Fs = [np.array(F, dtype=np.float64) for _ in range(count)]
    off = [np.zeros(2, dtype=np.int64) for _ in range(count)]
    iv = [[np.zeros(cap, dtype=np.int32) for _ in range(count)] for _ in range(4)]
    val = [np.zeros(cap) for _ in range(count)]
    pa = lambda arrays: (C.c_void_p * count)(*[a.ctypes.data for a in arrays])
    ns, bs = np.full(count, n, dtype=np.int64), np.full(count, bags.shape[1], dtype=np.int64)
    _lib.check(_lib.lib().mhs_gbm_grow_many(count, pa([Xf] * count), pa([y] * count), ns.ctypes.data, p, pa(list(bags)), bs.ctypes.data, 1,
                                            depth, minobs, C.c_double(shrinkage), 0, pa(Fs), None, pa(off), pa(iv[0]), pa(val), pa(iv[1]),
                                            pa(iv[2]), pa(iv[3])))
    out = []
    for k in range(count):
        nn = int(off[k][1])
        out.append(({"tree_offsets": off[k], "split_var": iv[0][k][:nn], "split_val": val[k][:nn], "left": iv[1][k][:nn],
                     "right": iv[2][k][:nn], "missing": iv[3][k][:nn]}, Fs[k]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(xi.GBM_LATER))
def test_gbm_later_trees_bit_equal(hip, name):
    """a later tree (first_call = 0) from a caller-supplied integer-valued F: F = round(y / 2), and y minus a random
    integer field in +-3"""
    X, y, F, bags, depth, minobs = xi.gbm_later_case(name)
    refs = _gbm_reference_trees(X, y - F, bags, depth, minobs)
    got = _grow_from(X, y, F, bags, depth, minobs)
    _gbm_check("later-" + name, y, [g[0] for g in got], refs)
    tol = 1e-12 * np.abs(y).max()
    for (_, Fk), ref in zip(got, refs):
        assert np.abs(Fk - (F + gbm_ref.tree_values(ref, X))).max() <= tol


# ---------------------------------------------------------------- earth: the same rule in its forward pass

@pytest.mark.gpu
def test_earth_duplicate_columns_go_to_the_first(hip):
    """"variables ascending; only a strictly greater reduction replaces the best": columns 0 and 1 appended again as
    variables 5 and 6 go through identical arithmetic, so their reductions are exactly equal, and no term may use 5 or 6"""
    X, y = ei.small()
    X = np.column_stack([X, X[:, :2]])
    ref = earth_ref.fit(X, y)
    assert np.all(ref["forward"]["dirs"][:, 5:] == 0) and np.any(ref["forward"]["dirs"][:, :2] != 0)
    m = hip.models.Earth.fit(X, y)
    rec = {k: getattr(m, k) for k in ("selected", "rss_per_subset", "gcv_per_subset", "prune_terms", "forward", "rss", "gcv", "rsq", "grsq")}
    rec.update(coef=m.params["coef"], dirs=m.params["dirs"], cuts=m.params["cuts"])
    decided = earth_ref.check_model(X, y, rec)
    print("earth: steps decided inside the window: device", decided, "reference", ref["window_decided"])
    assert decided <= ref["window_decided"]
    assert np.all(m.forward["dirs"][:, 5:] == 0) and np.any(m.forward["dirs"][:, :2] != 0)
