"""Inputs on which every sum of the tree fits is EXACT, shared by test_tree_ties_host.py and test_tree_ties_gpu.py.

The device adds a segment's c y (forest) or z (gbm) in 64-row steps with a log-depth scan inside the step, the references
(rf_ref.py, gbm_ref.py) add sequentially, and that difference is why the other tests grant near-ties a tolerance.  With an
integer-valued response, integer in-bag counts and integer residuals every partial sum is an integer below 2^53 (a float64
holds it exactly), so the order of addition does not matter, and the criterion is the same operations in the same order on
both sides: on these inputs the device must reproduce the float64 reference bit for bit, exact ties included.
:func:`assert_exact` is that precondition; every test calls it.

The tables: the bundled example's own station table (integer climate response, INT2S covariates: full of exact ties), a
synthetic table rounded to 1 decimal with a small-integer response, and large tables past the rows the kernels keep on
chip.  RF_CASES / GBM_CASES name every case of the GPU module; the host module shows per case that the deliberately wrong
tie-breaks of the references change its trees."""
import os
import re

import numpy as np

import gbm_inputs as gi
import rf_inputs as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_exact(values, counts=1):
    """The precondition of an exact comparison: every value is an integer, and n max(count) max|value| < 2^53, so every
    partial sum of count * value over any subset, in any order, is an integer that float64 represents."""
    v = np.asarray(values, dtype=np.float64)
    c = np.asarray(counts)
    assert np.all(np.isfinite(v)) and np.all(v == np.rint(v)), "a value is not an integer"
    assert np.all(c == np.rint(c)) and c.min() >= 0, "a count is not a non-negative integer"
    assert float(v.size) * float(c.max()) * float(np.abs(v).max()) < 2.0 ** 53, "a partial sum may pass 2^53"


def _integer_mean(y):
    """y with one value (the largest) lowered so that sum(y) % n == 0"""
    y = np.array(y, dtype=np.float64)
    y[int(np.argmax(y))] -= float(y.sum() % y.size)
    assert y.sum() % y.size == 0
    return y


def real_table(integer_mean=False):
    """X, y of gbm_inputs.stations(): n = 813, p = 4 (slope, TWI integer-valued; LONG, LAT), integer response 63 .. 261.
    ``integer_mean``: one value (the largest) is lowered by sum(y) % n, so that mean(y) is exactly the integer 219."""
    X, y, _ = gi.stations()
    return X, (_integer_mean(y) if integer_mean else y.copy())


def tied_table(n, p, seed):
    """n rows, p predictors rounded to 1 decimal, a small-integer response with mean exactly 0."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, p)), 1)
    y = np.rint(2.0 * np.sin(X[:, 0]) + X[:, 1] * X[:, min(2, p - 1)]) + rng.integers(-1, 2, size=n)
    y[:int(y.sum() % n)] -= 1.0
    y -= y.sum() // n
    assert y.sum() == 0
    return X, y


def big_table(n, p=4, seed=60, above=None):
    """n rows beyond what a kernel keeps on chip: predictors rounded to 1 decimal, a small-integer response, mean 0.
    ``above``: the response is 0 wherever variable 0 is not > above -- a best-first tree then spends its splits inside
    that tail, where the nodes get small enough for exact ties."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, p)), 1)
    y = np.rint(2.0 * np.cos(X[:, 0]) * X[:, 1] + X[:, 2]) + rng.integers(-1, 2, size=n)
    if above is not None:
        y = y * (X[:, 0] > above)
    y[:int(y.sum() % n)] -= 1.0
    y -= y.sum() // n
    assert y.sum() == 0
    return X, y


def rf_lds_rows():
    """RF_LDS_ROWS, read from the source as test_rf_fit_gpu.py does"""
    src = open(os.path.join(ROOT, "machisplin_amd", "csrc", "rf_fit.hip")).read()
    return int(re.search(r"constexpr int RF_LDS_ROWS = (\d+);", src).group(1))


# ---- the forest's cases: name -> (table, n_trees, mtry, nodesize, all in-bag counts 1)
RF_CASES = {
    "real-mtry1-ns5": (("real",), 10, 1, 5, False),
    "real-mtry2-ns5": (("real",), 10, 2, 5, False),
    "real-mtry4-ns1": (("real",), 10, 4, 1, False),
    "tied-300": (("tied", 300, 5, 70), 10, 5, 5, False),
    "tied-200": (("tied", 200, 5, 71), 10, 5, 5, False),           # the second model of the rf_fit_many call
    "edge-63": (("tied", 63, 3, 72), 4, 3, 1, True),
    "edge-64": (("tied", 64, 3, 73), 4, 3, 1, True),
    "edge-65": (("tied", 65, 3, 74), 4, 3, 1, True),
    "edge-129": (("tied", 129, 3, 75), 4, 3, 1, True),
    "past-lds": (("big",), 2, 2, 20, False),
}
RF_EDGES = ("edge-63", "edge-64", "edge-65", "edge-129")


def _table(spec):
    if spec[0] == "real":
        return real_table()
    if spec[0] == "tied":
        return tied_table(*spec[1:])
    return big_table(rf_lds_rows() + 8)


def rf_case(name):
    """(X, y, inbag, seeds, mtry, nodesize) of a forest case"""
    spec, n_trees, mtry, nodesize, ones = RF_CASES[name]
    X, y = _table(spec)
    inbag, seeds = ri.bags_for(y.size, n_trees, 80 + sorted(RF_CASES).index(name))
    if ones:
        inbag = np.ones_like(inbag)
    assert_exact(y, inbag)
    return X, y, inbag, seeds, mtry, nodesize


# ---- gbm's first-tree cases: name -> (table, bags, the bags' seed, depth, minobs); z = y - mean(y), an integer mean
# On the real table 25 splits of 406 bag rows never reach a node small enough for a within-variable tie (no tree changed at
# any n.minobsinnode, measured with the reference), and at n.minobsinnode = 10 hardly a cross-variable one: its two cases
# run at the kernel's largest depth, 64, and n.minobsinnode 3 and 5, where the reference alone meets the admission
# conditions of test_tree_ties_host.py.
GBM_CASES = {
    "real-minobs3": (("real",), 40, 90, 64, 3),
    "real-minobs5": (("real",), 40, 90, 64, 5),
    "tied-minobs10": (("tied", 300, 5, 70), 40, 93, 25, 10),
    "tied-minobs1": (("tied", 300, 5, 70), 40, 93, 25, 1),
    "tied-depth64": (("tied", 300, 5, 70), 40, 93, 64, 1),         # most trees hinge on the terminal-list order
    # one model, ONE tree: the response lives where variable 0 > 2 and the depth is the kernel's largest (64), so that
    # this single tree meets small nodes -- all three wrong tie-breaks change it (test_tree_ties_host.py)
    "large-n": (("large",), 1, 61, 64, 1),
}
GBM_LARGE_N = 20000                # the rows no longer fit on chip (GF_LDS_ROWS = 8192 in csrc/gbm_fit.hip)


def gbm_case(name):
    """(X, y, bags, depth, minobs) of a first-tree case: 40 bags of n / 2, every one the first tree of a model of its own"""
    spec, n_bags, bag_seed, depth, minobs = GBM_CASES[name]
    if spec[0] == "real":
        X, y = real_table(integer_mean=True)
    elif spec[0] == "tied":
        X, y = tied_table(*spec[1:])
    else:
        X, y = big_table(GBM_LARGE_N, seed=61, above=2.0)
    assert y.sum() % y.size == 0
    assert_exact(y)
    assert_exact(y - y.sum() / y.size)
    return X, y, gi.bags_for(y.size, n_bags, bag_seed), depth, minobs


# ---- gbm's later trees: the real table from a caller-supplied integer-valued F
GBM_LATER = {"half": (96, 64, 3), "random": (97, 64, 5)}       # name -> (the bags' seed, depth, minobs)


def gbm_later_case(name):
    """(X, y, F, bags, depth, minobs): F = round(y / 2), or y minus a random integer field in +-3 (z takes seven
    distinct values: equal improvements are frequent)"""
    bag_seed, depth, minobs = GBM_LATER[name]
    X, y = real_table()
    if name == "half":
        F = np.rint(y / 2.0)
    else:
        F = y - np.random.default_rng(95).integers(-3, 4, size=y.size)
    assert_exact(y)
    assert_exact(F)
    assert_exact(y - F)
    return X, y, F, gi.bags_for(y.size, 40, bag_seed), depth, minobs


def device_scan(a):
    """The running sums of ``a`` in the DEVICE's order, written in numpy: 64-row steps, inside a step a log-depth
    Hillis-Steele scan over the lanes (fit_wave_scan), the steps chained by a carried sum (carry + lane prefix)."""
    a = np.asarray(a)
    out = np.empty_like(a)
    carry = a.dtype.type(0)
    for base in range(0, a.size, 64):
        v = np.zeros(64, dtype=a.dtype)
        m = min(64, a.size - base)
        v[:m] = a[base:base + m]
        o = 1
        while o < 64:
            v[o:] = v[o:] + v[:-o].copy()
            o <<= 1
        out[base:base + m] = (carry + v)[:m]
        carry = carry + v[63]
    return out
