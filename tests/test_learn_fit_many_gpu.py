"""GPU: the batched learner fits -- mhs_nnet_fit_many (a layer's nnet models in one launch, a workgroup per model) and
mhs_svr_fit_many (a layer's ksvm models: Gram matrices in one arena, the SMO a workgroup per model) through
models.nnet_fit_many / models.ksvm_fit_many.  The yardstick is twofold: every model of a batch equals the single fit
(Nnet.fit / Ksvm.fit, pinned by tests/test_learn_fit_gpu.py) BIT FOR BIT, whatever shares the launch and however the
batch is packed; and the batch meets oracle/fit.py within the margins of tests/test_learn_fit_gpu.py.  The data
generator is that file's ``_data``."""
import ctypes as C

import numpy as np
import pytest

from oracle import ensemble as oe
from oracle import fit as of

pytestmark = pytest.mark.gpu


def _data(n=300, p=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p)) * np.array([1, 2, 3, 1, 5.0, 2, 1])[:p] + np.arange(p)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rng.normal(size=n)
    return rng, X, y


def _same_nnet(a, b):
    assert np.array_equal(a.wts, b.wts) and a.value == b.value and a.counts == b.counts and a.fail == b.fail


def _same_ksvm(a, b):
    assert np.array_equal(a.beta, b.beta) and a.n_iter == b.n_iter
    for key in ("b", "sigma", "y_center", "y_scale"):
        assert a.params[key] == b.params[key], key
    for key in ("x_center", "x_scale", "alpha", "sv"):
        assert np.array_equal(a.params[key], b.params[key]), key


def test_nnet_batched_equals_alone(hip):
    """Row counts below one row per thread (37), exactly one wave (64), either side of the 256 threads (255, 257) and the
    full set (400); a short run, so the oracle's iterates can be followed as tests/test_learn_fit_gpu.py follows them."""
    rng, X, y = _data(400, 5, seed=16)
    H, p = 10, 5
    sets = []
    for k, m in enumerate((37, 64, 255, 257, 400)):
        rows = np.sort(np.random.default_rng([16, k]).choice(400, m, replace=False))
        sets.append((X[rows], y[rows], np.random.default_rng([17, k]).uniform(-0.7, 0.7, (p + 1) * H + H + 1)))
    Xs, ys, w0 = [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets]
    batch = hip.models.nnet_fit_many(Xs, ys, w0, maxit=25)
    alone = [hip.models.Nnet.fit(a, b, w, maxit=25) for a, b, w in sets]
    back = hip.models.nnet_fit_many(Xs[::-1], ys[::-1], w0[::-1], maxit=25)[::-1]
    for k, (a, b, w) in enumerate(sets):
        _same_nnet(batch[k], alone[k])
        _same_nnet(back[k], alone[k])
        assert np.array_equal(batch[k].wts0, w)
        t = (b - b.min()) / (b - b.min()).max()
        ow, val, nf, ng, fail = of.nnet_fit(a, t, w, maxit=25)
        dw, dv = np.abs(batch[k].wts - ow).max() / np.abs(ow).max(), abs(batch[k].value - val) / val
        print("nnet batch model %d (n = %d): counts %s oracle %s, weights %.2e, value %.2e" % (k, a.shape[0], batch[k].counts, (nf, ng), dw, dv))
        assert batch[k].counts == (nf, ng) and batch[k].fail == fail
        assert dw < 1e-8 and dv < 1e-10
        assert np.abs(batch[k].predict_points(a[:16]) - alone[k].predict_points(a[:16])).max() == 0.0


@pytest.mark.parametrize("p", [3, 5, 7])
def test_nnet_batched_full_fit(hip, p):
    """maxit = 10000 as V73:249: a batch of three (p is per call) converges by vmmin's own test."""
    H, n = 10, 300
    sets = [_data(n, p, seed=40 + 3 * p + k)[1:] for k in range(3)]
    fits = hip.models.nnet_fit_many([s[0] for s in sets], [s[1] for s in sets], seed=p)
    for k, ((X, y), m) in enumerate(zip(sets, fits)):
        assert m.fail == 0
        assert np.array_equal(m.wts0, np.random.default_rng([p, k]).uniform(-0.7, 0.7, (p + 1) * H + H + 1))
        t = (y - y.min()) / (y - y.min()).max()
        v, _ = of.nnet_value_grad(m.wts, X, t, H)
        assert abs(v - m.value) < 1e-9 * v
        want = oe.predict_nnet(oe.nnet_model(m.wts, p, H, (y - y.min()).max(), y.min()), X[:50])
        assert np.abs(m.predict_points(X[:50]) - want).max() < 1e-12 * np.abs(y).max()


KSVM_CASES = [(97, 0.05), (300, 0.2), (1500, 0.5), (2049, 0.5)]      # 2049: one station past the 256-thread layout


@pytest.fixture(scope="module")
def ksvm_batch(hip):
    sets = [_data(n, 5, seed=n)[1:] for n, _ in KSVM_CASES]
    sig = [s for _, s in KSVM_CASES]
    batch = hip.models.ksvm_fit_many([s[0] for s in sets], [s[1] for s in sets], sig)
    return sets, sig, batch


def test_ksvm_batched_equals_alone(hip, ksvm_batch):
    sets, sig, batch = ksvm_batch
    for (X, y), s, m in zip(sets, sig, batch):
        _same_ksvm(m, hip.models.Ksvm.fit(X, y, s))
        assert m.sigma == s
        Z = (X - X.mean(0)) / X.std(0, ddof=1)
        t = (y - y.mean()) / y.std(ddof=1)
        K = of.rbf_gram(Z, s)
        ob, orho, _ = of.svr_smo(K, t)
        kkt, dk, db = of.svr_kkt_violation(K, t, m.beta), np.abs(K @ (m.beta - ob)).max(), abs(m.params["b"] - orho)
        print("ksvm batch n = %d: kkt %.3e, |K dbeta| %.3e, |db| %.3e, iterations %d" % (y.size, kkt, dk, db, m.n_iter))
        assert kkt < 1e-3 * 1.001
        assert dk < 5e-3 and db < 5e-3
        assert np.abs(m.predict_points(X[:32]) - oe.predict(m.params, X[:32])).max() < 1e-11 * np.abs(y).max()


def test_ksvm_packing_does_not_change_a_bit(hip, ksvm_batch):
    """A Gram budget of 8 * 1500^2 + 1 bytes: {97, 300} share a launch (1500 no longer fits beside them), 1500 has one of
    its own, and 2049, larger than the budget, goes alone."""
    sets, sig, batch = ksvm_batch
    packed = hip.models.ksvm_fit_many([s[0] for s in sets], [s[1] for s in sets], sig, gram_budget=8 * 1500 ** 2 + 1)
    for a, b in zip(packed, batch):
        _same_ksvm(a, b)


def _tie_sets():
    sets = []
    for n in (240, 2100):
        rng, X, _ = _data(n=n, p=4, seed=3)
        sets.append((X, rng.integers(180, 190, n).astype(float)))
    return sets


def test_ksvm_batched_ties(hip):
    """Integer responses: ties in every reduction, in a 256-thread launch's neighbour (240) and past it (2100)."""
    sets = _tie_sets()
    batch = hip.models.ksvm_fit_many([s[0] for s in sets], [s[1] for s in sets], 0.3)
    for (X, y), m in zip(sets, batch):
        _same_ksvm(m, hip.models.Ksvm.fit(X, y, 0.3))
        Z = (X - X.mean(0)) / X.std(0, ddof=1)
        _, _, oit = of.svr_smo(of.rbf_gram(Z, 0.3), (y - y.mean()) / y.std(ddof=1))
        print("ksvm ties n = %d: iterations %d, oracle %d" % (y.size, m.n_iter, oit))
        assert abs(m.n_iter - oit) <= 0.05 * oit


def test_ksvm_mixed_routes(hip):
    """One model a block holds and one that needs the cooperative grid (8300 > 8192), in one call."""
    sets = []
    for n in (300, 8300):
        rng = np.random.default_rng(5)
        X = rng.uniform(-2, 2, (n, 3))
        sets.append((X, np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.2 * X[:, 2] + 0.3 * rng.normal(size=n)))
    Xf = [np.asfortranarray(s[0]) for s in sets]
    ns = np.array([300, 8300], dtype=np.int64)
    sig = np.array([1.0, 1.0])
    beta, xc, xs = [np.zeros(n) for n in ns], [np.empty(3) for _ in ns], [np.empty(3) for _ in ns]
    b, yc, ys = np.empty(2), np.empty(2), np.empty(2)
    it, status = np.zeros(2, dtype=np.int64), np.full(2, -1, dtype=np.int32)
    pa = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    from machisplin_amd import _lib
    rc = _lib.lib().mhs_svr_fit_many(2, pa(Xf), pa([s[1] for s in sets]), ns.ctypes.data, 3, sig.ctypes.data, 1.0, 0.1, 1e-3, 0, 0,
                                     pa(beta), b.ctypes.data, pa(xc), pa(xs), yc.ctypes.data, ys.ctypes.data, it.ctypes.data,
                                     status.ctypes.data)
    assert rc == 0 and status.tolist() == [0, 0]
    for k, (X, y) in enumerate(sets):
        m = hip.models.Ksvm.fit(X, y, 1.0)
        assert np.array_equal(beta[k], m.beta) and b[k] == m.params["b"] and it[k] == m.n_iter
        assert np.array_equal(xc[k], m.params["x_center"]) and np.array_equal(xs[k], m.params["x_scale"])
        assert yc[k] == m.params["y_center"] and ys[k] == m.params["y_scale"]


def test_ksvm_no_convergence_fills_every_output(hip):
    """max_iter = 1: both models stop after one step with status 1, the call reports it and still hands everything back."""
    from machisplin_amd import _lib
    sets = _tie_sets()
    Xf = [np.asfortranarray(s[0]) for s in sets]
    ns = np.array([s[1].size for s in sets], dtype=np.int64)
    sig = np.array([0.3, 0.3])
    beta, xc, xs = [np.zeros(n) for n in ns], [np.empty(4) for _ in ns], [np.empty(4) for _ in ns]
    b, yc, ys = np.full(2, np.nan), np.empty(2), np.empty(2)
    it, status = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    pa = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    rc = _lib.lib().mhs_svr_fit_many(2, pa(Xf), pa([s[1] for s in sets]), ns.ctypes.data, 4, sig.ctypes.data, 1.0, 0.1, 1e-3, 1, 0,
                                     pa(beta), b.ctypes.data, pa(xc), pa(xs), yc.ctypes.data, ys.ctypes.data, it.ctypes.data,
                                     status.ctypes.data)
    assert rc != 0 and b"model 0" in _lib.lib().mhs_last_error()
    assert status.tolist() == [1, 1] and it.tolist() == [1, 1] and np.isfinite(b).all()
    for k, (X, y) in enumerate(sets):
        Z = (X - X.mean(0)) / X.std(0, ddof=1)
        want, _, _ = of.svr_smo(of.rbf_gram(Z, 0.3), (y - y.mean()) / y.std(ddof=1), max_iter=1)
        assert np.array_equal(np.flatnonzero(beta[k]), np.flatnonzero(want))
        assert np.allclose(beta[k][np.flatnonzero(want)], want[np.flatnonzero(want)], rtol=1e-12)
        assert yc[k] == y.mean() or abs(yc[k] - y.mean()) < 1e-12 * abs(y.mean())
