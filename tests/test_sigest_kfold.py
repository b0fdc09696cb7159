"""CPU: the two host rules Step 1 needs beside the device fits -- models.sigest (kernlab's automatic kernel width as
ksvm applies it) and cv.kfold (machisplin.kfold, V73:1553-1573) -- against values worked out here from their
definitions."""
import numpy as np
import pytest

from machisplin_amd import cv, models


def _type7(d, q):
    """R's default quantile (type 7) of the values d at probability q"""
    d = np.sort(np.asarray(d, dtype=float))
    h = (d.size - 1) * q
    lo = int(np.floor(h))
    hi = min(lo + 1, d.size - 1)
    return d[lo] + (h - lo) * (d[hi] - d[lo])


def test_sigest_from_the_definition():
    X = np.array([[1.0, 10.0], [2.0, 14.0], [4.0, 11.0], [7.0, 19.0], [8.0, 12.0], [11.0, 30.0]])
    index = np.array([0, 1, 2, 3, 4, 5, 0, 3])
    index2 = np.array([5, 4, 2, 0, 1, 1, 3, 3])            # pairs 2-2 and 3-3 coincide: d == 0, dropped
    n = 6
    mean = X.sum(0) / n
    sd = np.sqrt(((X - mean) ** 2).sum(0) / (n - 1))
    z = (X - mean) / sd
    d = [float(((z[i] - z[j]) ** 2).sum()) for i, j in zip(index, index2) if i != j]
    assert len(d) == 6
    want = np.array([1.0 / _type7(d, 0.9), 1.0 / _type7(d, 0.5), 1.0 / _type7(d, 0.1)])
    got = models.sigest(X, index, index2)
    assert got.shape == (3,) and np.allclose(got, want, rtol=1e-13, atol=0)
    assert got[0] < got[1] < got[2]
    # the drawn pairs: m = floor(frac n) of them, the same seed gives the same value, another seed other pairs
    rng = np.random.default_rng(3)
    Y = rng.normal(size=(41, 3))
    a, b = models.sigest(Y, seed=7), models.sigest(Y, seed=7)
    assert np.array_equal(a, b)
    g = np.random.default_rng(7)
    i1, i2 = g.integers(0, 41, 20), g.integers(0, 41, 20)
    assert np.array_equal(a, models.sigest(Y, i1, i2))
    assert not np.array_equal(a, models.sigest(Y, seed=[7, 1]))


def _half_even(x):
    f = np.floor(x)
    r = x - f
    if r > 0.5 or (r == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


def test_kfold_group_sizes_and_rounding():
    # 813 rows (the bundled example), 10 folds: diff(round(c(0, 81.3 * 1:9, 813))), R rounding half to even
    edges = [_half_even(x) for x in [0.0] + [813 / 10 * j for j in range(1, 10)] + [813.0]]
    sizes = [b - a for a, b in zip(edges[:-1], edges[1:])]
    assert edges[5] == 406 and sizes == [81, 82, 81, 81, 81, 82, 81, 81, 82, 81]         # 406.5 -> 406
    lab = cv.kfold(813, 10)
    assert lab.shape == (813,) and np.bincount(lab)[1:].tolist() == sizes and lab.min() == 1 and lab.max() == 10
    assert np.array_equal(lab, cv.kfold(813, 10, seed=0)) and not np.array_equal(lab, cv.kfold(813, 10, seed=1))
    assert not np.array_equal(lab, np.sort(lab))                                         # permuted, not in blocks
    # 25 rows: the edges 2.5, 5, 7.5, ... round to 2, 5, 8, 10, 12, 15, 18, 20, 22 (2.5 -> 2, 7.5 -> 8, 12.5 -> 12)
    assert [_half_even(2.5), _half_even(7.5), _half_even(12.5), _half_even(17.5), _half_even(22.5)] == [2, 8, 12, 18, 22]
    assert np.bincount(cv.kfold(25, 10))[1:].tolist() == [2, 3, 3, 2, 2, 3, 3, 2, 2, 3]
    assert np.array_equal(cv.kfold(7, 1), np.ones(7, dtype=int))
    with pytest.raises(ValueError):
        cv.kfold(5, 10)
