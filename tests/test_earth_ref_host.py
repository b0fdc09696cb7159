"""CPU: the yardstick of the earth fit tests guards itself.  On every committed input the float64 and the
extended-precision pass of tests/earth_ref.py make the same choices and NO step of the reference is decided inside the
tie window -- the condition test_earth_fit_gpu.py relies on when it allows the device no window-decided step either."""
import numpy as np
import pytest

import earth_inputs as ei
import earth_ref


@pytest.fixture(scope="module")
def fits():
    return {name: (gen(), earth_ref.fit(*gen())) for name, gen in ei.COMMITTED.items()}


@pytest.mark.parametrize("name", sorted(ei.COMMITTED))
def test_float64_and_longdouble_agree(fits, name):
    (X, y), a = fits[name]
    b = earth_ref.fit(X, y, acc=np.longdouble)
    assert earth_ref.same_structure(a, b)
    assert a["window_decided"] == 0 and b["window_decided"] == 0
    rel = abs(a["rss"] - b["rss"]) / b["rss"]
    print(name, "terms", len(a["coef"]), "of", len(a["selected"]), "stop", a["forward"]["stop"], "rss rel diff", rel)
    assert rel <= 1e-12
    # the reference passes its own certificate, with no step inside the window
    assert earth_ref.check_model(X, y, a) == 0


@pytest.mark.parametrize("kw", [dict(nk=7), dict(minspan=1, endspan=1)])
def test_other_arguments(kw):
    for gen in (ei.small, ei.stations):
        X, y = gen()
        a = earth_ref.fit(X, y, **kw)
        assert a["window_decided"] == 0 and earth_ref.check_model(X, y, a, **kw) == 0
        if "nk" in kw:
            assert len(a["selected"]) <= 7 and a["forward"]["stop"] == "nk"


def test_hinge_recovery():
    """a noiseless sum of two hinges at 0.4 and 0.6: the cuts are the nearest eligible knots"""
    X, y = ei.two_hinges()
    a = earth_ref.fit(X, y)
    ms, es = earth_ref.spans(*X.shape)
    terms = earth_ref.terms_from(a["dirs"], a["cuts"])
    for v, want in ((0, 0.4), (1, 0.6)):
        xs = np.sort(X[:, v], kind="stable")
        knots = xs[earth_ref.knot_positions(xs, ms, es)]
        dist = np.abs(knots - want)
        nearest = set(knots[dist <= dist.min() + 1e-12])           # two knots when they straddle the hinge evenly
        cuts = {t for (u, d, t) in terms if u == v and d in (1, -1)}
        assert len(cuts) == 1 and cuts <= nearest, (v, cuts, nearest)
    assert a["rsq"] > 0.999


def test_pruning_against_lstsq(fits):
    (X, y), a = fits["stations"]
    fd, fc = a["forward"]["dirs"], a["forward"]["cuts"]
    B = earth_ref.basis(X, fd, fc)
    for k in range(1, B.shape[1] + 1):
        cols = a["prune_terms"][k - 1, :k]
        e = y - B[:, cols] @ np.linalg.lstsq(B[:, cols], y, rcond=None)[0]
        assert abs(a["rss_per_subset"][k - 1] - e @ e) <= 1e-10 * (e @ e)
    # sizes shrink by one term, the RSS never falls, the selected size has the smallest GCV
    assert np.all(np.diff(a["rss_per_subset"]) <= 1e-12 * a["rss_per_subset"][0])
    assert a["gcv"] == a["gcv_per_subset"].min()


def test_spans_and_knots():
    assert earth_ref.spans(813, 7) == (6, 10) and earth_ref.spans(813, 7, 1, 1) == (1, 1)
    xs = np.array([0.0, 0.0, 0.1, 0.1, 0.1, 0.2, 0.3, 0.3, 0.4, 0.5])
    assert list(earth_ref.knot_positions(xs, 1, 2)) == [2, 5, 6]      # 3, 4 and 7 repeat their left neighbour
    assert list(earth_ref.knot_positions(xs, 3, 2)) == [2, 5]
    assert earth_ref.default_nk(7) == 21 and earth_ref.default_nk(32) == 65
