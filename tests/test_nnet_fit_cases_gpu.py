"""GPU: nnet_bfgs_kernel<P> (R's vmmin in one workgroup, csrc/learn_fit.hip) at every P = 1 .. 12 it is instantiated for, at
the row counts where its row loop (256 threads) and its reduction (four waves of 64) change shape, and through the branches
of vmmin that a fit takes in practice.  The cases and their data are tests/nnet_fit_cases.py; on the CPU,
tests/test_nnet_fit_cases_host.py has shown for each of them that the oracle's path does not depend on the order of its sums
(over the rows, over the hidden units) and that the listed branch is taken.

Lock-step cases (the device follows the oracle iterate for iterate): counts and `fail` equal to the oracle's, the weights
within 1e-8 of max |w| (the project's bound, tests/test_learn_fit_gpu.py), the value within VALUE_BOUND = 1e-8 relative --
100 x the largest change of the oracle's value when its sums are reordered (1.2e-10, profiles/nnet_fit_bounds.txt), cut at the
ceiling of 1e-8.  Measured on an MI355X: weights within 5.1e-11, values within 7.5e-11.

  * every p = 1 .. 12 at maxit = 25, n over {1, 12, 63, 64, 65, 255, 256, 257, 400, 1100}, p = 12 at n = 400 and n = 1100;
  * the `D1 <= 0` reset and the clamped sigmoid (saturated starts in +-8 and +-30; two of the 25-iteration cases reset too);
  * the periodic reset (p = 1, NW = 31, after 63 gradients);
  * stop by abstol with the no-progress restart (n = 1 and n = 12: the net interpolates), stop by reltol (a saturated
    start at p = 12), each run to vmmin's own end, fail = 0;
  * maxit = 0; a start without a finite value.
The uphill branch is not covered: no start reaches it on the CPU (see the host test).

One row: nnet's response scaling (V73:455-459) divides by max(resp - min) = 0, so Nnet.fit has no finite start there (as in
R); the n = 1 cases go through mhs_nnet_fit itself with the response as it is.

Whole fits (default maxit, thousands of gradients: not to be followed in lock-step) are checked as the existing full-fit test
checks them: fail = 0, the returned value is the oracle's criterion at the returned weights to 1e-9, no worse than the
25-iteration run, the same bits on repeat, and the same bits from nnet_fit_many with another model of the same p in the
launch (nnet_fit_many takes one p per call: three launches, not one)."""
import ctypes as C

import numpy as np
import pytest

import nnet_fit_cases as nc
from oracle import fit as of

pytestmark = pytest.mark.gpu


def _device_fit(hip, case, maxit=None):
    """(w, value, counts, fail) of the device fit of a case"""
    from machisplin_amd import _lib
    X, t, w0 = nc.data(case)
    maxit = case.maxit if maxit is None else maxit
    if case.n > 1:
        m = hip.models.Nnet.fit(X, t, w0, maxit=maxit)          # t has min 0 and max 1: the scaling leaves every bit
        return m.wts, m.value, m.counts, m.fail
    Xf, w = np.asfortranarray(X), w0.copy()
    val, counts, fail = C.c_double(), (C.c_int * 2)(), C.c_int()
    _lib.check(_lib.lib().mhs_nnet_fit(Xf.ctypes.data, t.ctypes.data, case.n, case.p, nc.H, w.ctypes.data, maxit, 1e-4, 1e-8,
                                       C.byref(val), counts, C.byref(fail)))
    return w, val.value, (counts[0], counts[1]), fail.value


@pytest.mark.parametrize("case", nc.LOCKSTEP + nc.BRANCH, ids=lambda c: c.name)
def test_device_follows_the_oracle(hip, case):
    w, val, cnt, fail, trace = nc.oracle_run(case)
    gw, gval, gcnt, gfail = _device_fit(hip, case)
    dw, dv = np.abs(gw - w).max() / np.abs(w).max(), abs(gval - val) / val
    print("%s: oracle counts %s fail %d value %.9e | device counts %s fail %d value %.9e | dw %.2e dv %.2e"
          % (case.name, cnt, fail, val, gcnt, gfail, gval, dw, dv))
    assert tuple(gcnt) == cnt and gfail == fail
    assert dw <= nc.WEIGHT_BOUND
    assert dv <= nc.VALUE_BOUND
    if case.branch:
        assert trace[case.branch] >= 1


def test_maxit_zero_returns_the_initial_value(hip):
    for case in (nc.LOCKSTEP[3], nc.LOCKSTEP[2]):              # through Nnet.fit, and one row through the C entry point
        X, t, w0 = nc.data(case)
        w, val, cnt, fail = _device_fit(hip, case, maxit=0)
        want = of.nnet_value_grad(w0, X, t, nc.H)[0]
        assert np.array_equal(w, w0) and tuple(cnt) == (0, 0) and fail == 0
        assert abs(val - want) <= 1e-13 * want


def test_a_start_without_a_finite_value_raises_and_the_library_goes_on(hip):
    case = nc.LOCKSTEP[3]
    X, t, w0 = nc.data(case)
    for bad_value in (np.inf, np.nan):
        bad = w0.copy()
        bad[-1] = bad_value
        with pytest.raises(hip.MhsError, match="not finite"):
            hip.models.Nnet.fit(X, t, bad, maxit=5)
        with pytest.raises(hip.MhsError, match="model 1: the initial value is not finite"):
            hip.models.nnet_fit_many([X, X], [t, t], [w0, bad], maxit=5)
    with np.errstate(invalid="ignore"), pytest.raises(hip.MhsError, match="non-finite response"):
        hip.models.Nnet.fit(X[:1], t[:1], w0, maxit=5)          # one row through the response scaling: 0 / 0
    w, val, cnt, fail, _ = nc.oracle_run(case)
    gw, gval, gcnt, gfail = _device_fit(hip, case)
    assert tuple(gcnt) == cnt and gfail == fail and np.abs(gw - w).max() <= nc.WEIGHT_BOUND * np.abs(w).max()


@pytest.mark.parametrize("case", nc.WHOLE, ids=lambda c: c.name)
def test_whole_fits(hip, case):
    X, t, w0 = nc.data(case)
    short = hip.models.Nnet.fit(X, t, w0, maxit=25)
    full = hip.models.Nnet.fit(X, t, w0)
    crit = of.nnet_value_grad(full.wts, X, t, nc.H)[0]
    print("%s: counts %s fail %d value %.9e criterion %.9e (25 iterations: %.9e)" % (case.name, full.counts, full.fail, full.value, crit, short.value))
    assert full.fail == 0 and full.counts[0] >= full.counts[1] > 25
    assert abs(crit - full.value) <= 1e-9 * crit
    assert short.fail == 1 and full.value <= short.value
    again = hip.models.Nnet.fit(X, t, w0)
    assert np.array_equal(again.wts, full.wts) and again.counts == full.counts and again.value == full.value and again.fail == 0
    # with another model of the same p beside it in the launch, in either order
    other = case._replace(seed=case.seed + 1, n=case.n + 1)
    X2, t2, w2 = nc.data(other)
    alone2 = hip.models.Nnet.fit(X2, t2, w2)
    for order in ((0, 1), (1, 0)):
        sets = [(X, t, w0), (X2, t2, w2)]
        batch = hip.models.nnet_fit_many([sets[k][0] for k in order], [sets[k][1] for k in order], [sets[k][2] for k in order])
        for k, got in zip(order, batch):
            want = (full, alone2)[k]
            assert np.array_equal(got.wts, want.wts) and got.counts == want.counts and got.value == want.value and got.fail == want.fail


def test_thirteen_predictors_are_refused(hip):
    """nnet_bfgs_kernel is instantiated for P = 1 .. 12: p = 13 is an error that names the limit, not another code path"""
    rng = np.random.default_rng(13)
    X, y = rng.normal(size=(40, 13)), rng.uniform(size=40)
    w0 = rng.uniform(-0.7, 0.7, nc.nw(13))
    with pytest.raises(hip.MhsError, match="12"):
        hip.models.Nnet.fit(X, y, w0, maxit=5)
    with pytest.raises(hip.MhsError, match="12"):
        hip.models.nnet_fit_many([X, X], [y, y], [w0, w0], maxit=5)
    case = nc.LOCKSTEP[11]                                      # p = 12 right after: the largest instantiation still fits
    w, val, cnt, fail, _ = nc.oracle_run(case)
    gw, gval, gcnt, gfail = _device_fit(hip, case)
    assert tuple(gcnt) == cnt and gfail == fail and np.abs(gw - w).max() <= nc.WEIGHT_BOUND * np.abs(w).max()
