"""Host (no GPU): pins the case table of tests/test_nnet_fit_cases_gpu.py (tests/nnet_fit_cases.py) on the oracle.

The device runs R's vmmin with its sums in another order than numpy's: over the rows (256 threads, a butterfly per wave, four
waves) and over the ten hidden units (one after the other; numpy's dot product is free to do otherwise).  A case can be
followed iterate for iterate only if the oracle's own path does not depend on that order, so every lock-step and branch case
is run here as it is and five times with its rows and its hidden units permuted -- the same problem: vmmin starts from the
identity, so relabelling the units relabels every iterate.  (The rows alone are not enough: a case of one row has no order
of rows, and two such cases that ended after a 27-evaluation line search at rounding level differed from the device by one
evaluation; under a permutation of the units they differ from themselves, and have other seeds now.)

  * the counts (fncount, grcount) and `fail` are the same in every order (an unstable case gets another seed, none is
    dropped);
  * the branch a case is listed for is taken, and its maxit lies just past the event;
  * the largest relative change of a weight (dw) and of the value (dv) is recorded: profiles/nnet_fit_bounds.txt, written
    by `python tests/test_nnet_fit_cases_host.py`.  Measured: dw <= 8.4e-11, dv <= 1.2e-10.  The device test holds the
    weights to the project's 1e-8 of max |w| (some 100 x dw) and the value to VALUE_BOUND = 100 x dv but no more than 1e-8,
    which is 1e-8; this file pins that to the measurement.

The uphill branch of vmmin (a search direction with t'g >= 0) is not in the table: none of these cases reaches it, nor did
any of 100 saturated starts (p in {2, 4, 6, 12}, +-8 and +-30, 120 iterations each) -- B stays positive definite through
the `D1 > 0` guard, so only rounding can produce one.  test_no_case_takes_the_uphill_branch says so for the table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":           # run as a script, without the suite's conftest: the same two path entries
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import nnet_fit_cases as nc          # noqa: E402
from oracle import ensemble as oe    # noqa: E402
from oracle import fit as of         # noqa: E402

CASES = nc.LOCKSTEP + nc.BRANCH


def test_the_table_covers_every_p_and_every_n():
    assert {c.p for c in nc.LOCKSTEP} == set(range(1, 13))
    assert {c.n for c in nc.LOCKSTEP} == {1, 12, 63, 64, 65, 255, 256, 257, 400, 1100}
    assert {(12, 400), (12, 1100)} <= {(c.p, c.n) for c in nc.LOCKSTEP}
    assert all(c.maxit == 25 and c.amp == 0.7 for c in nc.LOCKSTEP)
    assert [(c.p, c.n) for c in nc.WHOLE] == [(1, 65), (2, 63), (12, 400)] and all(c.maxit == 10000 for c in nc.WHOLE)
    assert len({c.name for c in CASES + nc.WHOLE}) == len(CASES + nc.WHOLE)
    for c in CASES + nc.WHOLE:
        X, t, w0 = nc.data(c)
        assert X.shape == (c.n, c.p) and w0.size == nc.nw(c.p) and np.abs(w0).max() <= c.amp
        assert (c.n == 1 and 0.0 < t[0] < 1.0) or (t.min() == 0.0 and t.max() == 1.0)
        assert c.n == 1 or np.array_equal((t - t.min()) / (t - t.min()).max(), t)      # Nnet.fit's scaling leaves every bit


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_counts_do_not_depend_on_the_order_of_the_sums(case):
    w, val, cnt, fail, trace, stable, dw, dv = nc.measure(case)
    print("%s: counts %s fail %d value %.6e dw %.2e dv %.2e" % (case.name, cnt, fail, val, dw, dv))
    assert stable, "counts or fail change when the sums are reordered: the case needs another seed"
    assert np.isfinite(w).all() and np.isfinite(val) and val > 0.0
    assert fail == int(cnt[1] >= case.maxit)
    assert dw <= nc.WEIGHT_BOUND / 10          # the device's 1e-8 leaves an order of magnitude above the oracle's own spread


@pytest.mark.parametrize("case", nc.BRANCH, ids=lambda c: c.name)
def test_the_listed_branch_is_taken(case):
    w, val, cnt, fail, trace = nc.measure(case)[:5]
    assert trace.get(case.branch, 0) >= 1, trace
    first = trace[case.branch + "_at"][0]
    if case.maxit < 10000:                     # cut just past the event: the event, then at most two more gradients
        assert first < case.maxit <= first + 2 and fail == 1 and trace["maxit"] == 1
    else:                                      # runs to vmmin's own stop
        assert fail == 0 and "maxit" not in trace and cnt[0] < 50
        assert trace["no_progress_restart"] == 1        # the stop, one restart from the identity, the stop again
    if case.branch == "periodic_reset":
        assert first == 2 * nc.nw(case.p) + 2 and "d1_reset" not in trace       # gradcount - ilast > 2 NW with ilast = 1
    if case.branch == "stop_abstol":
        assert val <= 1e-4
    if case.branch == "stop_reltol":
        assert val > 1e-4


@pytest.mark.parametrize("case", [c for c in nc.BRANCH if c.amp > 1.0], ids=lambda c: c.name)
def test_saturated_starts_reach_the_clamped_sigmoid(case):
    """nnet's sigmoid returns exactly 0 / 1 beyond |z| = 15: at the start and at the returned weights most hidden units sit
    there on most rows, on both sides."""
    X, t, w0 = nc.data(case)
    for w in (w0, nc.measure(case)[0]):
        W1 = w[:(case.p + 1) * nc.H].reshape(nc.H, case.p + 1)
        z = W1[:, 0][None, :] + X @ W1[:, 1:].T
        assert (z > 15.0).mean() > 0.1 and (z < -15.0).mean() > 0.1
        h = oe._nnet_sigmoid(z)
        assert (h[z > 15.0] == 1.0).all() and (h[z < -15.0] == 0.0).all()


def test_no_case_takes_the_uphill_branch():
    for case in CASES:
        assert "uphill" not in nc.measure(case)[4], case.name


def test_lockstep_cases_see_step_reductions_and_a_d1_reset():
    """the 25-iteration cases are no easy descents: every one of more than one row rejects trial steps, two reset B"""
    for case in nc.LOCKSTEP:
        trace = nc.measure(case)[4]
        assert trace.get("step_reduction", 0) >= 1, case.name
    assert sum("d1_reset" in nc.measure(c)[4] for c in nc.LOCKSTEP) >= 2


def test_the_trace_changes_no_result():
    for case in (nc.LOCKSTEP[4], nc.BRANCH[0], nc.BRANCH[2]):
        X, t, w0 = nc.data(case)
        plain = of.nnet_fit(X, t, w0, maxit=case.maxit)
        trace = {}
        traced = of.nnet_fit(X, t, w0, maxit=case.maxit, trace=trace)
        assert np.array_equal(plain[0], traced[0]) and plain[1:] == traced[1:]
        assert set(k for k in trace if not k.endswith("_at")) <= set(of.TRACE_EVENTS)
        assert all(len(trace[k + "_at"]) == trace[k] for k in trace if not k.endswith("_at") and k != "step_reduction")


def test_maxit_zero_and_a_start_without_a_finite_value():
    case = nc.LOCKSTEP[3]
    X, t, w0 = nc.data(case)
    w, val, nf, ng, fail = of.nnet_fit(X, t, w0, maxit=0)
    assert np.array_equal(w, w0) and (nf, ng, fail) == (0, 0, 0) and val == of.nnet_value_grad(w0, X, t, nc.H)[0]
    bad = w0.copy()
    bad[-1] = np.inf
    with np.errstate(invalid="ignore"), pytest.raises(ValueError, match="not finite"):
        of.nnet_fit(X, t, bad, maxit=5)


def test_the_value_bound_is_the_measured_one():
    """VALUE_BOUND = 100 x the largest dv over the lock-step and branch cases, at most 1e-8; the committed table says the same."""
    text, worst_w, worst_v = nc.bounds_table()
    print(text)
    assert min(100.0 * worst_v, 1e-8) <= nc.VALUE_BOUND <= 1e-8
    assert nc.VALUE_BOUND <= 2.0 * 100.0 * worst_v, "the bound is no longer the measured one: rewrite profiles/nnet_fit_bounds.txt"
    with open(os.path.join(ROOT, "profiles", "nnet_fit_bounds.txt")) as f:
        committed = f.read()
    assert "VALUE_BOUND = %.0e" % nc.VALUE_BOUND in committed and "WEIGHT_BOUND = %.0e" % nc.WEIGHT_BOUND in committed
    for case in CASES:
        assert any(line.startswith(case.name + " ") for line in committed.splitlines()), case.name


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "nnet_fit_bounds.txt"), "w") as out:
        out.write(nc.bounds_table()[0])
