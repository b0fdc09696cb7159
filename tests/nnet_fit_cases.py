"""The case table of the nnet-fit tests: tests/test_nnet_fit_cases_host.py pins it on the CPU (the oracle's counts do not
depend on the order of the rows, the listed branch of vmmin is taken), tests/test_nnet_fit_cases_gpu.py runs it on the
device.  A case is data (n rows, p predictors, a response in [0, 1] as V73:455-459 leaves it), a start and a maxit."""
import collections

import numpy as np

from oracle import fit as of

H = 10          # size = 10 (V73:249, V73:463)
_SCALE = np.array([1, 2, 3, 1, 5.0, 2, 1, 0.5, 4, 1.5, 2.5, 1])

WEIGHT_BOUND = 1e-8        # of max |w|: the project's bound for a device fit that follows the oracle iterate for iterate
VALUE_BOUND = 1e-8         # of the value: 100 x the largest change under a reordering of the sums (1.2e-10, see
                           # profiles/nnet_fit_bounds.txt), which the ceiling of 1e-8 cuts

Case = collections.namedtuple("Case", "name p n seed amp maxit branch")

# every p = 1 .. 12 once at least, every n of {1, 12, 63, 64, 65, 255, 256, 257, 400, 1100} (the row loop strides by 256
# threads and reduces over four waves of 64), p = 12 with n = 400 and n = 1100; 25 iterations from a start in +-0.7
LOCKSTEP = [Case("p%d_n%d" % (p, n), p, n, seed, 0.7, 25, None)
            for p, n, seed in [(1, 255, 161), (2, 65, 265), (3, 1, 303), (4, 64, 464), (5, 12, 512), (6, 63, 663), (7, 256, 762),
                               (8, 257, 863), (9, 1100, 933), (10, 400, 1012), (11, 63, 1163), (12, 400, 1212), (12, 1100, 1233),
                               (12, 1, 1204)]]

# one branch of vmmin each; maxit lies just past the event (the host test reads the iteration off the oracle's trace)
BRANCH = [
    Case("saturated_p4", 4, 100, 57, 8.0, 20, "d1_reset"),            # |z| > 15 on most rows: the clamped sigmoid, flat directions
    Case("saturated_p6", 6, 64, 54, 30.0, 12, "d1_reset"),
    Case("periodic_p1", 1, 63, 18, 0.7, 66, "periodic_reset"),        # NW = 31: B is reset after 2 NW + 1 = 63 gradients
    Case("reltol_p12", 12, 64, 41, 8.0, 10000, "stop_reltol"),        # a saturated start that ends on reltol after 11 gradients
    Case("abstol_n1_p3", 3, 1, 33, 0.7, 10000, "stop_abstol"),        # one row, twelve rows: the net interpolates, the value
    Case("abstol_n12_p5", 5, 12, 51, 0.7, 10000, "stop_abstol"),      # falls below abstol = 1e-4 and vmmin restarts once
]

# default maxit: too long to follow iterate for iterate
WHOLE = [Case("whole_p1_n65", 1, 65, 165, 0.7, 10000, None), Case("whole_p2_n63", 2, 63, 263, 0.7, 10000, None),
         Case("whole_p12_n400", 12, 400, 1200 + 400 % 97, 0.7, 10000, None)]


def nw(p):
    return (p + 1) * H + H + 1


def data(case):
    """(X, t, w0): n x p predictors on the scales of raster covariates, the response scaled to [0, 1] (min 0, max 1, so
    that the scaling of Nnet.fit leaves every bit of it; one row: a single value inside (0, 1)), the start in +-amp."""
    rng = np.random.default_rng(case.seed)
    X = rng.normal(size=(case.n, case.p)) * _SCALE[:case.p] + np.arange(case.p)
    y = np.sin(X[:, 0]) + 0.3 * X[:, -1] + 0.1 * rng.normal(size=case.n)
    t = (y - y.min()) / (y - y.min()).max() if case.n > 1 else np.array([0.37])
    w0 = rng.uniform(-case.amp, case.amp, nw(case.p))
    return X, t, w0


def oracle_run(case, perm=None, maxit=None, units=None):
    """the oracle's fit of the case, rows in the order `perm`, hidden units in the order `units` (the start relabelled, the
    returned weights labelled back): (w, value, (fncount, grcount), fail, trace)"""
    X, t, w0 = data(case)
    if perm is not None:
        X, t = X[perm], t[perm]
    split = (case.p + 1) * H
    if units is not None:
        w0 = np.concatenate([w0[:split].reshape(H, case.p + 1)[units].ravel(), w0[split:split + 1], w0[split + 1:][units]])
    trace = {}
    w, val, nf, ng, fail = of.nnet_fit(X, t, w0, size=H, maxit=case.maxit if maxit is None else maxit, trace=trace)
    if units is not None:
        back = np.argsort(units)
        w = np.concatenate([w[:split].reshape(H, case.p + 1)[back].ravel(), w[split:split + 1], w[split + 1:][back]])
    return w, val, (nf, ng), fail, trace


def permutations(case, count=3):
    """`count` pairs (an order of the rows, an order of the hidden units)"""
    rng = np.random.default_rng(case.seed + 7919)
    return [(rng.permutation(case.n), rng.permutation(H)) for _ in range(count)]


_MEASURED = {}


def measure(case, count=5):
    """The oracle on the case as it is and `count` times with its rows and its hidden units in another order -- the same
    problem (vmmin starts from the identity, so relabelling the units relabels every iterate) with the sums over the rows and
    over the units in another order, which is what differs on the device: (w, value, counts, fail, trace, stable, dw, dv)
    with stable = the counts and fail are the same in every order, dw / dv = the largest change of a weight relative to
    max |w| / of the value relative to the value.  Computed once per case and process."""
    if case.name not in _MEASURED:
        w, val, cnt, fail, trace = oracle_run(case)
        stable, dw, dv = True, 0.0, 0.0
        for perm, units in permutations(case, count):
            w2, v2, c2, f2, _ = oracle_run(case, perm, units=units)
            stable = stable and c2 == cnt and f2 == fail
            dw = max(dw, float(np.abs(w2 - w).max() / np.abs(w).max()))
            dv = max(dv, abs(v2 - val) / val)
        _MEASURED[case.name] = (w, val, cnt, fail, trace, stable, dw, dv)
    return _MEASURED[case.name]


def bounds_table():
    """the text of profiles/nnet_fit_bounds.txt"""
    rows, worst_w, worst_v = [], 0.0, 0.0
    for case in LOCKSTEP + BRANCH:
        w, val, cnt, fail, trace, stable, dw, dv = measure(case)
        worst_w, worst_v = max(worst_w, dw), max(worst_v, dv)
        rows.append("%-16s p=%-2d n=%-4d maxit=%-5d counts=(%d, %d) fail=%d value=%.6e stable=%s dw=%.1e dv=%.1e" %
                    (case.name, case.p, case.n, case.maxit, cnt[0], cnt[1], fail, val, stable, dw, dv))
    head = ["nnet fit (vmmin): sensitivity of the oracle to the order of its sums: 5 permutations of the rows and of the hidden units per case",
            "(tests/nnet_fit_cases.py; written by `python tests/test_nnet_fit_cases_host.py`)",
            "dw = largest change of a weight / max |w|, dv = largest change of the value / value", ""]
    tail = ["", "largest dw = %.1e  (the weights are held to WEIGHT_BOUND = %.0e of max |w|, the bound of tests/test_learn_fit_gpu.py)" % (worst_w, WEIGHT_BOUND),
            "largest dv = %.1e  (the value is held to VALUE_BOUND = %.0e relative: 100 x the largest dv, rounded up to one digit," % (worst_v, VALUE_BOUND),
            "                     but no larger than 1e-8)"]
    return "\n".join(head + rows + tail) + "\n", worst_w, worst_v
