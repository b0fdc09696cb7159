"""The inputs of the gbm growth tests, shared by test_gbm_ref_host.py (which shows that their tree structures do not
hinge on the summation order) and test_gbm_fit_gpu.py (which then compares structures exactly)."""
import os

import numpy as np

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg1_extdata.npz")


def bags_for(n, n_trees, seed, size=None):
    """One generator, a fresh permutation per tree: ``default_rng(seed).permutation(n)[:size]`` drawn n_trees times."""
    rng = np.random.default_rng(seed)
    size = n // 2 if size is None else size
    return np.stack([rng.permutation(n)[:size] for _ in range(n_trees)]).astype(np.int32)


def short():
    """n = 300, p = 5, 40 trees, bags of 150."""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(300, 5))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rng.normal(size=300)
    return X, y, bags_for(300, 40, 1, 150)


def stations():
    """The 813-station table of the bundled example: slope and TWI at the station cells (INT2S: integer-valued, many
    ties), LONG, LAT; response = the first climate column.  Rows off the rasters or on NoData are dropped."""
    z = np.load(FIX)
    xmin, ymax, xres, yres, nrow, ncol = z["geom"]
    tab = z["sampling"]
    col = np.floor((tab[:, 0] - xmin) / xres).astype(np.int64)
    row = np.floor((ymax - tab[:, 1]) / yres).astype(np.int64)
    ok = (col >= 0) & (col < int(ncol)) & (row >= 0) & (row < int(nrow)) & np.isfinite(tab[:, 2])
    col, row, tab = col[ok], row[ok], tab[ok]
    slope = z["slope"][row, col].astype(np.float64)
    twi = z["TWI"][row, col].astype(np.float64)
    keep = (slope != float(z["nodata"])) & (twi != float(z["nodata"]))
    X = np.column_stack([slope, twi, tab[:, 0], tab[:, 1]])[keep]
    y = tab[keep, 2]
    return X, y, bags_for(y.size, 40, 2)


def long_models(count=10, n=3600, p=7, n_trees=500):
    """``count`` models of n rows (the size of a CV fold's training set, V73:228-232), bag fraction 0.5."""
    out = []
    for k in range(count):
        rng = np.random.default_rng([7, k])
        X = rng.normal(size=(n, p))
        y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.2 * np.abs(X[:, 3]) + 0.1 * rng.normal(size=n)
        out.append((X, y, bags_for(n, n_trees, [8, k])))
    return out


def large(n=20000, p=7, n_trees=30):
    """cfg5's final model size: beyond the rows the kernel keeps on chip."""
    rng = np.random.default_rng(11)
    X = rng.normal(size=(n, p))
    y = np.cos(X[:, 0]) * X[:, 1] + 0.3 * X[:, 2] + 0.1 * rng.normal(size=n)
    return X, y, bags_for(n, n_trees, 12)


LONG_EVERY = 25                       # the long test compares every 25th tree
LARGE_SAMPLED = (1, 7, 13, 22, 30)    # trees (1-based) of the large model that are compared
