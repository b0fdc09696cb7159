"""The seeded inputs of the random-forest growth tests, shared by test_rf_ref_host.py and test_rf_fit_gpu.py."""
import numpy as np


def bags_for(n, n_trees, seed):
    """(inbag, seeds): per tree a bootstrap of n rows with replacement as in-bag counts (n_trees x n int32), and one
    uint64 seed per tree for the variable draws."""
    rng = np.random.default_rng(seed)
    inbag = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(n_trees)]).astype(np.int32)
    return inbag, rng.integers(0, 2 ** 64, size=n_trees, dtype=np.uint64)


def small(n_trees=20):
    """n = 300, p = 5, continuous predictors."""
    rng = np.random.default_rng(30)
    X = rng.normal(size=(300, 5))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.1 * rng.normal(size=300)
    return (X, y) + bags_for(300, n_trees, 31)


def stations(n_trees=20):
    """n = 813 (the station count of the bundled example), p = 7, predictors rounded to 2 decimals: x has ties.  The
    response has no large offset: the criterion sl^2 / nl + sr^2 / nr - tot^2 / m carries an absolute rounding error of a
    few ulp of sum(c y^2), so the certificate's RELATIVE 1e-9 margins presume a best criterion that is not many orders
    below sum(c y^2) (with y = 250 + ... a node whose best criterion is 5e-4 is ordered by rounding alone)."""
    rng = np.random.default_rng(32)
    X = np.round(rng.normal(size=(813, 7)), 2)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.2 * np.abs(X[:, 3]) + 0.1 * rng.normal(size=813)
    return (X, y) + bags_for(813, n_trees, 33)


def plain(n, p, seed):
    """n rows, p continuous predictors, every row once in every bag's population of 1 (all counts 1 are made by the caller)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p))
    y = np.cos(X[:, 0]) * X[:, 1] + 0.2 * rng.normal(size=n)
    return X, y


def large(n=9000, p=4, n_trees=3):
    """Just past the rows the kernel keeps on chip (RF_LDS_ROWS = 8192 in csrc/rf_fit.hip)."""
    X, y = plain(n, p, 34)
    return (X, y) + bags_for(n, n_trees, 35)


def folds(n=600, p=5, nfolds=10):
    rng = np.random.default_rng(36)
    X = rng.normal(size=(n, p))
    y = 3.0 * np.sin(X[:, 0]) + X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=n)
    kfolds = np.resize(np.arange(1, nfolds + 1), n)[rng.permutation(n)]
    return X, y, kfolds
