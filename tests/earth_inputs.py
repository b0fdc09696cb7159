"""The seeded inputs of the earth (MARS) fit tests, shared by test_earth_ref_host.py and test_earth_fit_gpu.py."""
import numpy as np


def _response(X, rng, noise=0.1):
    """a sum of hinges, a linear term and a sine, with noise"""
    p = X.shape[1]
    return (3.0 * np.maximum(X[:, 0] - 0.4, 0.0) - 2.0 * np.maximum(0.6 - X[:, 1], 0.0) + 1.5 * X[:, min(2, p - 1)]
            + np.sin(5.0 * X[:, min(3, p - 1)]) + noise * rng.standard_normal(X.shape[0]))


def shape(n, p, seed, decimals=3):
    """x uniform on [0, 1] rounded to ``decimals`` (ties in x), y = _response"""
    rng = np.random.default_rng(seed)
    X = np.round(rng.uniform(0.0, 1.0, (n, p)), decimals)
    return X, _response(X, rng)


def small():
    return shape(300, 5, 1)


def stations():
    """n = 813: the station count of the bundled example"""
    return shape(813, 7, 2)


def tiny():
    return shape(64, 3, 3)


def wide():
    return shape(2000, 10, 4)


COMMITTED = {"small": small, "stations": stations, "tiny": tiny, "wide": wide}


def edge(n, p=3):
    """segments that end at, before and after a wave's 64 rows"""
    return shape(n, p, 100 + n)


def two_predictors():
    return shape(200, 2, 7)


def binary_variable():
    """variable 1 is 0 / 1 (no eligible knot: it enters linearly or not at all) and drives the response"""
    rng = np.random.default_rng(8)
    X = np.round(rng.uniform(0.0, 1.0, (240, 4)), 3)
    X[:, 1] = rng.integers(0, 2, 240)
    y = 2.0 * X[:, 1] + 3.0 * np.maximum(X[:, 0] - 0.5, 0.0) + 0.1 * rng.standard_normal(240)
    return X, y


def constant_variable():
    X, y = shape(240, 4, 9)
    X[:, 2] = 0.75
    return X, y


def linear_response():
    """y exactly linear in variable 1 (small integers over a power of two: every product and sum is exact)"""
    rng = np.random.default_rng(10)
    X = rng.integers(0, 1024, (200, 3)) / 1024.0
    return X, 2.0 + 3.0 * X[:, 1]


def heavy_ties():
    return shape(400, 3, 11, decimals=1)


def two_hinges(n=500, p=3):
    """a noiseless sum of two hinges, at 0.4 of variable 0 and 0.6 of variable 1"""
    rng = np.random.default_rng(12)
    X = np.round(rng.uniform(0.0, 1.0, (n, p)), 3)
    return X, 3.0 * np.maximum(X[:, 0] - 0.4, 0.0) + 2.0 * np.maximum(X[:, 1] - 0.6, 0.0)


def large(n):
    """just past the rows the kernel keeps on chip (EARTH_LDS_ROWS in csrc/earth_fit.hip)"""
    return shape(n, 3, 13)


def folds(n=600, p=5, nfolds=10):
    rng = np.random.default_rng(14)
    X = np.round(rng.uniform(0.0, 1.0, (n, p)), 3)
    y = _response(X, rng)
    kfolds = np.resize(np.arange(1, nfolds + 1), n)[rng.permutation(n)]
    return X, y, kfolds
