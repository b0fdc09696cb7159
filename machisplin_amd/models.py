"""Host-side mirror of the six fitted ensemble members as the hot path sees them:
flat parameter arrays in, ``terra::predict(rast_stack, model)`` /
``predict(model, data.frame)`` out (V73:447-619).  These classes wrap what the fitted R objects contain; the
six members all have a ``fit`` classmethod that runs on the device (gam, ksvm, nnet, gbm, randomForest, earth).  All
arithmetic runs in libmachisplin_hip.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from .raster import RasterStack


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


class Model:
    """Base: owns an ``mhs_model*``.  ``label`` is the reference's one-letter code
    (b, g, n, m, r, v -- V73:340-362)."""
    label = "?"

    def __init__(self, handle, p):
        self._h = handle
        self.p = int(p)

    def predict_points(self, X) -> np.ndarray:
        """predict(model, data.frame): X is n x p, columns in rast_stack order (covariates,
        LONG, LAT).  Used for the station residuals (V73:477-482, 501-505, ...)."""
        X = np.asfortranarray(np.asarray(X, dtype=np.float64))
        if X.ndim != 2 or X.shape[1] != self.p:
            raise ValueError(f"X must be n x {self.p}")
        if self._h is None:
            raise ValueError("this model holds a fit's record only: the evaluators take 2 .. 64 predictors")
        out = np.empty(X.shape[0])
        _lib.check(_lib.lib().mhs_predict_points(self._h, X.ctypes.data, X.shape[0], out.ctypes.data))
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None and _lib._lib is not None:      # (module globals are gone at interpreter exit)
            _lib._lib.mhs_model_free(h)
            self._h = None


def _fit_xy(X, y):
    """The rows of one fit: X as float64 in column-major order, y as float64, one response per row."""
    X, y = np.asfortranarray(np.asarray(X, dtype=np.float64)), _f64(y)
    if X.ndim != 2 or X.shape[0] != y.size:
        raise ValueError("X must be n x p with one response per row")
    return X, y


def _fit_inputs(Xs, ys):
    """The batch of a ``*_fit_many``: :func:`_fit_xy` of every model; one response vector per matrix, the same p throughout."""
    Xs, ys = list(Xs), list(ys)
    if not Xs or len(Xs) != len(ys):
        raise ValueError("need one response vector per predictor matrix")
    Xs, ys = map(list, zip(*[_fit_xy(X, y) for X, y in zip(Xs, ys)]))
    if any(X.shape[1] != Xs[0].shape[1] for X in Xs):
        raise ValueError("every X must have the same p")
    return Xs, ys


def _fit_generators(seed, count):
    """What seeds ``default_rng`` of each of ``count`` models: an int gives model k ``[seed, k]`` (a single model ``seed``
    itself); anything else is taken as one seed per model."""
    if np.ndim(seed) == 0:
        return [seed] if count == 1 else [[int(seed), k] for k in range(count)]
    return list(seed)


def _ptrs(arrs):
    """the addresses of a list of numpy arrays, as the ``T *const *`` arguments of the batched entry points take them"""
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _adopt(cls, handle, p):
    """a ``cls`` around an ``mhs_model*`` that the library returned (``cls.__init__``, the loader, is not run)"""
    m = cls.__new__(cls)
    Model.__init__(m, C.c_void_p(handle), p)
    return m


class Gam(Model):
    """mgcv::gam(resp ~ a + b + ...): no smooth terms (V73:195,600) => coefficients[p+1]."""
    label = "g"

    def __init__(self, coefficients):
        c = _f64(coefficients)
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_lm_load(c.ctypes.data, c.size - 1, C.byref(h)))
        super().__init__(h, c.size - 1)
        self.coefficients = c

    @classmethod
    def fit(cls, X, y) -> "Gam":
        """mgcv::gam(resp ~ a + b + ..., data) (V73:252, V73:600): least squares on the device (Householder QR of
        [1 X]).  X is n x p in rast_stack order, rows with NA already dropped (V73:154)."""
        X, y = _fit_xy(X, y)
        coef = np.empty(X.shape[1] + 1)
        _lib.check(_lib.lib().mhs_lm_fit(X.ctypes.data, y.ctypes.data, X.shape[0], X.shape[1], coef.ctypes.data))
        return cls(coef)


class Nnet(Model):
    """nnet::nnet(size=10, linout=TRUE) (V73:463) with the response un-scaling
    ``pred * max2.resp.f + min.resp.f`` (V73:469-470) folded in."""
    label = "n"

    def __init__(self, wts, p, size=10, max2_resp=1.0, min_resp=0.0):
        w = _f64(wts)
        if w.size != (p + 1) * size + size + 1:
            raise ValueError("wts has the wrong length for (p, size)")
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_nnet_load(w.ctypes.data, p, size, float(max2_resp), float(min_resp), C.byref(h)))
        super().__init__(h, p)

    @classmethod
    def fit(cls, X, y, wts0, size=10, maxit=10000, abstol=1e-4, reltol=1e-8) -> "Nnet":
        """nnet::nnet(mod.form, data = trainNN, size = 10, linout = TRUE, maxit = 10000) with the response scaling of
        V73:455-459 (resp - min, / max) around it, on the device (R's vmmin in one resident kernel).  wts0: the
        initial weights, nnet order (nnet draws runif(-0.7, 0.7)).  The object carries .wts, .value, .counts, .fail."""
        X, y = _fit_xy(X, y)
        n, p = X.shape
        w = _f64(wts0).copy()
        if w.size != (p + 1) * size + size + 1:
            raise ValueError("wts0 has the wrong length for (p, size)")
        mn, mx, ys = _nnet_scaled(y)
        val, counts, fail = C.c_double(), (C.c_int * 2)(), C.c_int()
        _lib.init()
        _lib.check(_lib.lib().mhs_nnet_fit(X.ctypes.data, ys.ctypes.data, n, p, int(size), w.ctypes.data, int(maxit), float(abstol),
                                           float(reltol), C.byref(val), counts, C.byref(fail)))
        return _nnet_object(w, p, size, mx, mn, val.value, counts, fail.value)


def _nnet_scaled(y):
    """V73:455-459: (min, max of resp - min, (resp - min) / max), the response nnet is trained on"""
    mn = float(y.min())
    mx = float((y - mn).max())
    return mn, mx, np.ascontiguousarray((y - mn) / mx)


def _nnet_object(w, p, size, mx, mn, value, counts, fail):
    if p >= 2:
        m = Nnet(w, p, size, mx, mn)
    else:       # the fit takes one predictor, the evaluators start at two (a covariate-free stack has LONG and LAT): the
        m = Nnet.__new__(Nnet)      # fit's record without a device model
        Model.__init__(m, None, p)
    m.wts, m.value, m.counts, m.fail = w, float(value), (int(counts[0]), int(counts[1])), int(fail)
    return m


def nnet_fit_many(Xs, ys, wts0=None, seed=0, size=10, maxit=10000, abstol=1e-4, reltol=1e-8):
    """:meth:`Nnet.fit` for several models (each its own rows and initial weights; the same p, size, maxit and
    tolerances) in ONE launch, a workgroup per model (mhs_nnet_fit_many): the shape of the ten fold models of V73:249 and
    of the final model of V73:463.  Every model gets the response scaling of V73:235-241 from its OWN rows, and equals
    :meth:`Nnet.fit` on those rows bit for bit, whatever shares the launch.  ``wts0``: one vector per model; ``None``
    draws model k's from ``default_rng(g_k).uniform(-0.7, 0.7, nw)`` -- nnet's ``rang``, NOT R's stream -- with ``g_k``
    as :func:`_fit_generators` derives it from ``seed`` (an int gives model k ``[seed, k]``, a single model ``seed``; or
    one seed per model).  Every model carries ``.wts``, ``.value``, ``.counts``, ``.fail`` and ``.wts0``."""
    Xs, ys = _fit_inputs(Xs, ys)
    count, p, size = len(Xs), Xs[0].shape[1], int(size)
    nw = (p + 1) * size + size + 1
    if wts0 is None:
        w0 = [np.random.default_rng(g).uniform(-0.7, 0.7, nw) for g in _fit_generators(seed, count)]
    else:
        w0 = [_f64(w).copy() for w in wts0]
        if len(w0) != count or any(w.size != nw for w in w0):
            raise ValueError("wts0 must hold one vector of the length for (p, size) per model")
    ws = [w.copy() for w in w0]
    mn, mx, ts = zip(*[_nnet_scaled(y) for y in ys])
    ns = _i64([X.shape[0] for X in Xs])
    val, counts, fail = np.empty(count), np.zeros(2 * count, dtype=np.int32), np.zeros(count, dtype=np.int32)
    _lib.init()
    _lib.check(_lib.lib().mhs_nnet_fit_many(count, _ptrs(Xs), _ptrs(ts), ns.ctypes.data, p, size, _ptrs(ws), int(maxit), float(abstol),
                                            float(reltol), val.ctypes.data, counts.ctypes.data, fail.ctypes.data))
    out = []
    for k in range(count):
        m = _nnet_object(ws[k], p, size, mx[k], mn[k], val[k], counts[2 * k:2 * k + 2], fail[k])
        m.wts0 = w0[k]
        out.append(m)
    return out


class Earth(Model):
    """earth::earth (V73:539): coefficients, dirs and cuts of the SELECTED terms."""
    label = "m"

    def __init__(self, coefficients, dirs, cuts):
        c, d, k = _f64(coefficients), _i32(dirs), _f64(cuts)
        if d.ndim != 2 or d.shape != k.shape or d.shape[0] != c.size:
            raise ValueError("dirs/cuts must be nterms x p")
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_earth_load(c.ctypes.data, d.ctypes.data, k.ctypes.data, d.shape[0], d.shape[1], C.byref(h)))
        super().__init__(h, d.shape[1])

    @classmethod
    def fit(cls, X, y, nk=None, thresh=0.001, penalty=2.0, minspan=0, endspan=0, nfold=0, fold=None, seed=0) -> "Earth":
        """earth::earth(mod.form, data, nfold = 10) (V73:250 per CV fold, V73:539 the final model) as that call drives
        it -- degree 1, backward pruning, penalty 2, thresh 0.001, nk = min(200, max(20, 2 p)) + 1, automatic spans --
        fitted on the device (mhs_earth_fit_many, a workgroup per model; the rule is stated in
        include/machisplin_hip.h, parity with R is not pinned).  The object carries ``.params`` (the ``kind = "earth"``
        dict of :func:`from_param_dict`), ``.forward`` (``dirs``, ``cuts``, ``rss``, ``stop``), ``.selected``,
        ``.rss_per_subset``, ``.gcv_per_subset``, ``.prune_terms`` (row k-1 = the forward terms kept at size k, -1
        padded), ``.rss``, ``.gcv``, ``.rsq`` and ``.grsq``.

        ``nfold > 0``: the ``nfold`` sub-models ride in the SAME launch as the main fit; sub-model f is trained on
        ``fold != f``.  ``fold``: 1-based labels, one per row; ``None`` draws a permutation of ``rep(1 .. nfold)`` from
        ``numpy.random.default_rng(seed)`` -- NOT R's RNG stream.  The model then carries ``.fold``, ``.cv_models``,
        ``.cv_rsq_folds`` (per fold ``1 - sum (y - yhat)^2 / sum (y - mean of the hold-out y)^2`` on the hold-out rows,
        through :meth:`predict_points`) and ``.cv_rsq`` (their mean).  This mirrors earth's ``cv.rsq`` in DEFINITION
        only: the folds are not earth's."""
        return earth_fit_many([X], [y], nk, thresh, penalty, minspan, endspan, nfold, None if fold is None else [fold], seed)[0]


EARTH_STOPS = {1: "constant", 2: "nk", 3: "none", 4: "thresh", 5: "rsq", 6: "grsq"}      # MHS_EARTH_STOP_*


def _earth_record(h, p):
    """mhs_earth_get: the sizes first, then every array"""
    lib = _lib.lib()
    ns, nf, stop = C.c_int(), C.c_int(), C.c_int()
    none = [None] * 11
    _lib.check(lib.mhs_earth_get(h, C.byref(ns), C.byref(nf), C.byref(stop), *none))
    S, M = ns.value, nf.value
    coef, cuts, fcuts = np.empty(S), np.empty((S, p)), np.empty((M, p))
    dirs, fdirs = np.empty((S, p), dtype=np.int32), np.empty((M, p), dtype=np.int32)
    frss, rss_sub, gcv_sub, stats = np.empty(M), np.empty(M), np.empty(M), np.empty(4)
    sel, pt = np.empty(M, dtype=np.int32), np.empty((M, M), dtype=np.int32)
    _lib.check(lib.mhs_earth_get(h, C.byref(ns), C.byref(nf), C.byref(stop), coef.ctypes.data, dirs.ctypes.data, cuts.ctypes.data,
                                 fdirs.ctypes.data, fcuts.ctypes.data, frss.ctypes.data, sel.ctypes.data, rss_sub.ctypes.data,
                                 gcv_sub.ctypes.data, pt.ctypes.data, stats.ctypes.data))
    return {"params": {"kind": "earth", "coef": coef, "dirs": dirs, "cuts": cuts},
            "forward": {"dirs": fdirs, "cuts": fcuts, "rss": frss, "stop": EARTH_STOPS[stop.value]},
            "selected": sel.astype(bool), "rss_per_subset": rss_sub, "gcv_per_subset": gcv_sub, "prune_terms": pt,
            "rss": float(stats[0]), "gcv": float(stats[1]), "rsq": float(stats[2]), "grsq": float(stats[3])}


def earth_fit_many(Xs, ys, nk=None, thresh=0.001, penalty=2.0, minspan=0, endspan=0, nfold=0, fold=None, seed=0):
    """:meth:`Earth.fit` for several models (each its own rows; the same p and arguments) in ONE device call, a workgroup
    per model: the shape of the ten fold models of V73:250.  With ``nfold > 0`` the call covers ``len(Xs) * (1 + nfold)``
    models.  ``fold``: one label vector per model; ``seed``: an int (model k draws its folds from
    ``default_rng([seed, k])``; a single model from ``default_rng(seed)``) or one per model."""
    Xs, ys = _fit_inputs(Xs, ys)
    count, p, nfold = len(Xs), Xs[0].shape[1], int(nfold)
    folds = [None] * count
    if nfold > 0:
        if nfold < 2:
            raise ValueError("nfold must be 0 or at least 2")
        gen = _fit_generators(seed, count)
        for k, X in enumerate(Xs):
            n = X.shape[0]
            if fold is None:
                f = np.resize(np.arange(1, nfold + 1), n)[np.random.default_rng(gen[k]).permutation(n)]
            else:
                f = np.asarray(fold[k])
                if f.shape != (n,) or f.min() < 1 or f.max() > nfold:
                    raise ValueError("fold must hold one label in 1 .. nfold per row")
            folds[k] = f
    # the launch list: every main model, then its nfold sub-models
    LX, Ly, owner = [], [], []
    for k in range(count):
        LX.append(Xs[k]); Ly.append(ys[k]); owner.append((k, 0))
        for f in range(1, nfold + 1):
            tr = np.flatnonzero(folds[k] != f)
            LX.append(np.asfortranarray(Xs[k][tr])); Ly.append(np.ascontiguousarray(ys[k][tr])); owner.append((k, f))
    total = len(LX)
    hs = (C.c_void_p * total)()
    ns = _i64([X.shape[0] for X in LX])
    _lib.init()
    _lib.check(_lib.lib().mhs_earth_fit_many(total, _ptrs(LX), _ptrs(Ly), ns.ctypes.data, p, 0 if nk is None else int(nk), float(thresh),
                                             float(penalty), int(minspan), int(endspan), hs))
    fitted = []
    for e in range(total):
        m = _adopt(Earth, hs[e], p)
        for key, val in _earth_record(m._h, p).items():
            setattr(m, key, val)
        fitted.append(m)
    out = []
    for k in range(count):
        m = fitted[k * (1 + nfold)]
        if nfold > 0:
            m.fold, m.cv_models = folds[k], fitted[k * (1 + nfold) + 1:(k + 1) * (1 + nfold)]
            Xc = np.ascontiguousarray(Xs[k])
            r2 = []
            for f, sub in enumerate(m.cv_models, start=1):
                ho = np.flatnonzero(folds[k] == f)
                d = ys[k][ho] - sub.predict_points(Xc[ho])
                dy = ys[k][ho] - np.mean(ys[k][ho])
                r2.append(1.0 - float(d @ d) / float(dy @ dy))
            m.cv_rsq_folds = np.array(r2)
            m.cv_rsq = float(np.mean(r2))
        out.append(m)
    return out


class Ksvm(Model):
    """kernlab::ksvm eps-svr / rbfdot / scaled=TRUE (V73:560)."""
    label = "v"

    def __init__(self, alpha, xmatrix, b, sigma, x_center, x_scale, y_center, y_scale):
        a, sv = _f64(alpha), _f64(xmatrix)
        xc, xs = _f64(x_center), _f64(x_scale)
        if sv.ndim != 2 or sv.shape[0] != a.size or xc.size != sv.shape[1] or xs.size != sv.shape[1]:
            raise ValueError("xmatrix must be nSV x p with matching alpha / scaling vectors")
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_svr_load(a.ctypes.data, sv.ctypes.data, sv.shape[0], sv.shape[1], float(b),
                                           float(sigma), xc.ctypes.data, xs.ctypes.data, float(y_center),
                                           float(y_scale), C.byref(h)))
        super().__init__(h, sv.shape[1])

    @classmethod
    def fit(cls, X, y, sigma, C_=1.0, epsilon=0.1, tol=1e-3, max_iter=0) -> "Ksvm":
        """kernlab::ksvm(mod.form, data) (V73:251, V73:560) on the device: eps-svr, rbfdot, scaled = TRUE, kernlab's
        defaults for C / epsilon / tol.  sigma is kpar$sigma (kernlab's automatic value is drawn by sigest() from a
        random half of the rows).  The fitted object carries .beta (n), .n_iter and the support-vector bundle."""
        X, y = _fit_xy(X, y)
        n, p = X.shape
        beta, xc, xs = np.empty(n), np.empty(p), np.empty(p)
        b, yc, ys, it = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        _lib.init()
        _lib.check(_lib.lib().mhs_svr_fit(X.ctypes.data, y.ctypes.data, n, p, float(sigma), float(C_), float(epsilon), float(tol),
                                          int(max_iter), beta.ctypes.data, C.byref(b), xc.ctypes.data, xs.ctypes.data,
                                          C.byref(yc), C.byref(ys), C.byref(it)))
        return _ksvm_object(X, beta, b.value, sigma, xc, xs, yc.value, ys.value, it.value)


def _ksvm_object(X, beta, b, sigma, xc, xs, yc, ys, n_iter):
    """the Ksvm of a fit's result: the support vectors are the rows with beta != 0, scaled as the fit scaled them"""
    sv = np.flatnonzero(beta != 0.0)
    Z = (np.ascontiguousarray(X)[sv] - xc) / xs
    m = Ksvm(beta[sv], Z, float(b), float(sigma), xc, xs, float(yc), float(ys))
    m.beta, m.n_iter, m.sv_index, m.sigma = beta, int(n_iter), sv, float(sigma)
    m.params = {"kind": "svr", "alpha": beta[sv], "sv": Z, "b": float(b), "sigma": float(sigma), "x_center": xc, "x_scale": xs,
                "y_center": float(yc), "y_scale": float(ys)}
    return m


def sigest(X, index=None, index2=None, seed=0, frac=0.5):
    """kernlab::sigest as ``ksvm(kpar = "automatic")`` applies it to the predictor matrix (host numpy, O(n)): the columns
    standardised (mean, sd with n - 1), ``m = floor(frac n)`` pairs of rows ``index`` / ``index2`` drawn with replacement,
    ``d`` their squared distances with the zeros dropped, and ``1 / quantile(d, [0.9, 0.5, 0.1])`` (linear interpolation,
    R's type 7) returned.  ksvm's automatic sigma is the mean of the first and the third value.  ``index`` / ``index2``
    ``None``: two draws of ``default_rng(seed).integers(0, n, m)`` -- NOT R's RNG stream, so the value is kernlab's rule
    on other pairs; parity with kernlab is not pinned."""
    X = np.ascontiguousarray(X, dtype=np.float64)          # one memory order: numpy's sums depend on it in the last bit
    if X.ndim != 2 or X.shape[0] < 2:
        raise ValueError("X must be n x p with at least two rows")
    n = X.shape[0]
    m = int(np.floor(frac * n))
    z = (X - X.mean(0)) / X.std(0, ddof=1)
    if index is None or index2 is None:
        rng = np.random.default_rng(seed)
        drawn = rng.integers(0, n, m), rng.integers(0, n, m)
        index = drawn[0] if index is None else index
        index2 = drawn[1] if index2 is None else index2
    index, index2 = np.asarray(index), np.asarray(index2)
    if index.shape != index2.shape or index.ndim != 1:
        raise ValueError("index and index2 must hold as many rows each")
    diff = z[index] - z[index2]
    d = np.sum(diff * diff, axis=1)
    d = d[d != 0.0]
    if d.size == 0:
        raise ValueError("every drawn pair of rows coincides")
    return 1.0 / np.quantile(d, [0.9, 0.5, 0.1])


def ksvm_fit_many(Xs, ys, sigma=None, seed=0, C_=1.0, epsilon=0.1, tol=1e-3, max_iter=0, gram_budget=0):
    """:meth:`Ksvm.fit` for several models (each its own rows and kernel width; the same C, epsilon, tol and max_iter) in
    ONE device call (mhs_svr_fit_many): the shape of the ten fold models of V73:251 and of the final model of V73:560.
    Models of up to 8 192 rows share three launches (Gram matrices in one arena, the SMO a workgroup per model, rho);
    ``gram_budget`` bounds that arena in bytes (0: half of the free device memory) and splits the batch into more
    launches where it must; larger models follow one by one.  Every model equals :meth:`Ksvm.fit` on its rows bit for
    bit, whatever the packing.  ``sigma``: a scalar (shared), one per model, or ``None`` -- kernlab's automatic value,
    ``mean(sigest(X_k, seed = g_k)[[0, 2]])`` with ``g_k`` as :func:`_fit_generators` derives it from ``seed`` (an int
    gives model k ``[seed, k]``, a single model ``seed``; or one seed per model), stored as ``.sigma``.  The models
    carry what :meth:`Ksvm.fit` sets, and ``.sigma``."""
    Xs, ys = _fit_inputs(Xs, ys)
    count, p = len(Xs), Xs[0].shape[1]
    if sigma is None:
        sig = np.array([float(np.mean(sigest(X, seed=g)[[0, 2]])) for X, g in zip(Xs, _fit_generators(seed, count))])
    elif np.ndim(sigma) == 0:
        sig = np.full(count, float(sigma))
    else:
        sig = _f64(sigma)
        if sig.shape != (count,):
            raise ValueError("sigma must be a scalar or hold one value per model")
    ns = _i64([X.shape[0] for X in Xs])
    beta = [np.empty(X.shape[0]) for X in Xs]
    xc, xs = [np.empty(p) for _ in Xs], [np.empty(p) for _ in Xs]
    b, yc, ysc = np.empty(count), np.empty(count), np.empty(count)
    it, status = np.zeros(count, dtype=np.int64), np.zeros(count, dtype=np.int32)
    _lib.init()
    _lib.check(_lib.lib().mhs_svr_fit_many(count, _ptrs(Xs), _ptrs(ys), ns.ctypes.data, p, sig.ctypes.data, float(C_), float(epsilon),
                                           float(tol), int(max_iter), int(gram_budget), _ptrs(beta), b.ctypes.data, _ptrs(xc), _ptrs(xs),
                                           yc.ctypes.data, ysc.ctypes.data, it.ctypes.data, status.ctypes.data))
    return [_ksvm_object(Xs[k], beta[k], b[k], sig[k], xc[k], xs[k], yc[k], ysc[k], it[k]) for k in range(count)]


class Gbm(Model):
    """gbm object evaluated at n.trees = best.trees, type="response" (V73:497)."""
    label = "b"

    def __init__(self, init_f, tree_offsets, split_var, split_val, left, right, missing, p):
        off = _i64(tree_offsets)
        sv, val, l, r, m = _i32(split_var), _f64(split_val), _i32(left), _i32(right), _i32(missing)
        if not (sv.size == val.size == l.size == r.size == m.size == off[-1]):
            raise ValueError("node arrays must all have tree_offsets[-1] entries")
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_gbm_load(float(init_f), off.size - 1, off.ctypes.data, sv.ctypes.data,
                                           val.ctypes.data, l.ctypes.data, r.ctypes.data, m.ctypes.data, p, C.byref(h)))
        super().__init__(h, p)
        self.n_trees = int(off.size - 1)

    def staged_predict_points(self, X, step: int) -> np.ndarray:
        """predict.gbm(model, X, n.trees = step, 2 step, ...) in one walk (mhs_gbm_staged_points): (n_trees // step, n);
        the hold-out predictions machisplin.gbm.step's tree-count search is run on (V73:1843, 1919)."""
        X = np.asfortranarray(np.asarray(X, dtype=np.float64))
        if X.ndim != 2 or X.shape[1] != self.p:
            raise ValueError("X must be n x p")
        out = np.empty((self.n_trees // int(step), X.shape[0]))
        if out.size:
            _lib.check(_lib.lib().mhs_gbm_staged_points(self._h, X.ctypes.data, X.shape[0], int(step), out.ctypes.data))
        return out


    @classmethod
    def fit(cls, X, y, n_trees, bags=None, seed=0, interaction_depth=25, shrinkage=0.01, bag_fraction=0.5,
            n_minobsinnode=10) -> "Gbm":
        """gbm::gbm(distribution = "gaussian", n.trees, interaction.depth, shrinkage, bag.fraction, n.minobsinnode) as
        machisplin.gbm.step calls it (V73:1772, V73:2101; tree.complexity = 25, learning.rate = 0.01, bag.fraction = 0.5
        at V73:247), grown on the device (mhs_gbm_grow_many).  ``bags``: (n_trees, bag_size) row indices, the rows
        tree t is grown on; ``None`` draws ``floor(bag_fraction * n)`` rows per tree without replacement from
        ``numpy.random.default_rng(seed)`` -- NOT R's RNG stream, so the trees are gbm's for these bags, not for
        R's ``set.seed``.  The object carries ``.params`` (the ``kind = "gbm"`` dict of :func:`from_param_dict`),
        ``.fit`` (the model's value on the training rows), ``.init_f`` and ``.error_reduction`` (node-aligned with
        ``params["split_var"]``: the improvement every split node won with, gbm's ErrorReduction; 0 at terminals)."""
        return gbm_fit_many([X], [y], n_trees, None if bags is None else [bags], seed, interaction_depth, shrinkage,
                            bag_fraction, n_minobsinnode)[0]

    def more(self, n_trees, bags=None) -> "Gbm":
        """gbm::gbm.more(model, n_trees) (V73:1908): a NEW model with n_trees further trees grown from this one's
        ``.fit``; bags as in :meth:`fit` (``None`` continues this model's generator)."""
        return gbm_more_many([self], n_trees, None if bags is None else [bags])[0]

    def relative_influence(self, n_trees=None) -> np.ndarray:
        """gbm's ``relative.influence(model, n.trees)``: per variable, the sum of ``.error_reduction`` over the split nodes
        of the first ``n_trees`` trees (all of them by default) that test it, added in tree order and then node order."""
        red = getattr(self, "error_reduction", None)
        if red is None:
            raise ValueError("relative influence needs a model grown by Gbm.fit / gbm_fit_many")
        n_trees = self.n_trees if n_trees is None else int(n_trees)
        if not 0 <= n_trees <= self.n_trees:
            raise ValueError("n_trees must lie in 0 .. %d" % self.n_trees)
        end = int(self.params["tree_offsets"][n_trees])
        var = np.asarray(self.params["split_var"][:end])
        out = np.zeros(self.p)
        np.add.at(out, var[var >= 0], red[:end][var >= 0])          # unbuffered: one addition per node, in node order
        return out

    def contributions(self):
        """``summary.gbm``'s rel.inf, what the reference stores as the member's $var.imp (V73:495; V73:2115, V73:2210):
        ``(100 * relative_influence() / its sum, the variables in descending order of it)`` -- the first array in
        VARIABLE order, ties of the order to the lower index.  All zeros when no tree has a split."""
        ri = self.relative_influence()
        tot = float(ri.sum())
        rel = 100.0 * ri / tot if tot > 0.0 else np.zeros(self.p)
        return rel, np.argsort(-rel, kind="stable")


def _gbm_bags(bags, rngs, ns, n_trees, bag_fraction):
    out = []
    for k, n in enumerate(ns):
        if bags is not None:
            b = _i32(bags[k])
            if b.ndim != 2 or b.shape[0] != n_trees:
                raise ValueError("bags must be n_trees x bag_size row indices")
        else:
            size = int(np.floor(bag_fraction * n))
            b = _i32(np.stack([rngs[k].permutation(n)[:size] for _ in range(n_trees)]))
        out.append(b)
    return out


def _gbm_grow(Xs, ys, Fs, bags, n_trees, depth, minobs, shrinkage):
    """mhs_gbm_grow_many_reduction; Fs None = the first call.  Returns per model (F, init_f, offsets, var, val, left, right,
    missing, error_reduction)."""
    count = len(Xs)
    p = Xs[0].shape[1]
    cap = n_trees * (3 * depth + 1)
    first = Fs is None
    Fs = [np.empty(X.shape[0]) for X in Xs] if first else [_f64(F).copy() for F in Fs]
    init = np.zeros(count)
    off = [np.zeros(n_trees + 1, dtype=np.int64) for _ in range(count)]
    var, left, right, miss = ([np.zeros(cap, dtype=np.int32) for _ in range(count)] for _ in range(4))
    val = [np.zeros(cap) for _ in range(count)]
    red = [np.zeros(cap) for _ in range(count)]
    ns = _i64([X.shape[0] for X in Xs])
    bs = _i64([b.shape[1] for b in bags])
    _lib.init()
    _lib.check(_lib.lib().mhs_gbm_grow_many_reduction(count, _ptrs(Xs), _ptrs(ys), ns.ctypes.data, p, _ptrs(bags), bs.ctypes.data,
                                                      int(n_trees), int(depth), int(minobs), float(shrinkage), int(first), _ptrs(Fs),
                                                      init.ctypes.data, _ptrs(off), _ptrs(var), _ptrs(val), _ptrs(left), _ptrs(right),
                                                      _ptrs(miss), _ptrs(red)))
    out = []
    for k in range(count):
        nn = int(off[k][-1])
        out.append((Fs[k], float(init[k]), off[k], var[k][:nn], val[k][:nn], left[k][:nn], right[k][:nn], miss[k][:nn], red[k][:nn]))
    return out


def _gbm_object(params, F, state, red):
    m = from_param_dict(params)
    m.params, m.fit, m.init_f, m._grow, m.error_reduction = params, F, params["init_f"], state, red
    return m


def gbm_fit_many(Xs, ys, n_trees, bags=None, seed=0, interaction_depth=25, shrinkage=0.01, bag_fraction=0.5,
                 n_minobsinnode=10):
    """:meth:`Gbm.fit` for several models (each its own rows) in ONE device call, a workgroup per model: the shape of
    machisplin.gbm.step's ten fold models (V73:1816-1919).  ``bags``: one (n_trees, bag_size) array per model; ``seed``:
    an int (model k draws from ``default_rng([seed, k])``; a single model from ``default_rng(seed)``) or one per model."""
    Xs, ys = _fit_inputs(Xs, ys)
    rngs = [np.random.default_rng(s) for s in _fit_generators(seed, len(Xs))] if bags is None else [None] * len(Xs)
    bags = _gbm_bags(bags, rngs, [X.shape[0] for X in Xs], int(n_trees), bag_fraction)
    res = _gbm_grow(Xs, ys, None, bags, int(n_trees), interaction_depth, n_minobsinnode, shrinkage)
    out = []
    for k, (F, init_f, off, var, val, left, right, miss, red) in enumerate(res):
        params = {"kind": "gbm", "init_f": init_f, "tree_offsets": off, "split_var": var, "split_val": val, "left": left,
                  "right": right, "missing": miss, "p": Xs[k].shape[1]}
        state = {"X": Xs[k], "y": ys[k], "rng": rngs[k], "depth": interaction_depth, "minobs": n_minobsinnode,
                 "shrinkage": shrinkage, "bag_fraction": bag_fraction}
        out.append(_gbm_object(params, F, state, red))
    return out


def gbm_more_many(models, n_trees, bags=None):
    """:meth:`Gbm.more` for several grown models (the same depth, shrinkage and n.minobsinnode) in ONE device call."""
    st = [getattr(m, "_grow", None) for m in models]
    if not st or any(s is None for s in st):
        raise ValueError("gbm.more needs models grown by Gbm.fit / gbm_fit_many")
    key = lambda s: (s["depth"], s["minobs"], s["shrinkage"], s["X"].shape[1])
    if any(key(s) != key(st[0]) for s in st):
        raise ValueError("the models must share p, interaction_depth, n_minobsinnode and shrinkage")
    if bags is None and any(s["rng"] is None for s in st):
        raise ValueError("a model grown from explicit bags needs explicit bags to continue")
    bags = _gbm_bags(bags, [s["rng"] for s in st], [s["X"].shape[0] for s in st], int(n_trees), st[0]["bag_fraction"])
    res = _gbm_grow([s["X"] for s in st], [s["y"] for s in st], [m.fit for m in models], bags, int(n_trees), st[0]["depth"],
                    st[0]["minobs"], st[0]["shrinkage"])
    out = []
    for m, s, (F, _, off, var, val, left, right, miss, red) in zip(models, st, res):
        q = m.params
        params = {"kind": "gbm", "init_f": q["init_f"], "tree_offsets": np.concatenate([q["tree_offsets"], q["tree_offsets"][-1] + off[1:]]),
                  "split_var": np.concatenate([q["split_var"], var]), "split_val": np.concatenate([q["split_val"], val]),
                  "left": np.concatenate([q["left"], left]), "right": np.concatenate([q["right"], right]),
                  "missing": np.concatenate([q["missing"], miss]), "p": q["p"]}
        out.append(_gbm_object(params, F, s, np.concatenate([m.error_reduction, red])))
    return out


class _ImportanceTable(np.ndarray):
    """What :func:`rf_importance_many` stores as ``model.importance``: the p x 2 array.  The attribute takes the place of
    the method :meth:`RandomForest.importance` on that model, so the array can still be called like it."""
    _model = None

    def __array_finalize__(self, obj):
        self._model = getattr(obj, "_model", None)

    def __call__(self, X, y, inbag=None, perm_seeds=None, n_perm=1, seed=0):
        m = self._model() if self._model is not None else None
        if m is None:
            raise ReferenceError("this importance table has outlived its forest: call RandomForest.importance on a live model")
        return RandomForest.importance(m, X, y, inbag, perm_seeds, n_perm, seed)


class RandomForest(Model):
    """randomForest regression forest (V73:517), prediction = mean over trees."""
    label = "r"

    def __init__(self, tree_offsets, left, right, status, best_var, split, node_pred, p):
        off = _i64(tree_offsets)
        l, r, st, bv = _i32(left), _i32(right), _i32(status), _i32(best_var)
        sp, npred = _f64(split), _f64(node_pred)
        if not (l.size == r.size == st.size == bv.size == sp.size == npred.size == off[-1]):
            raise ValueError("node arrays must all have tree_offsets[-1] entries")
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_rf_load(off.size - 1, off.ctypes.data, l.ctypes.data, r.ctypes.data, st.ctypes.data,
                                          bv.ctypes.data, sp.ctypes.data, npred.ctypes.data, p, C.byref(h)))
        super().__init__(h, p)

    @classmethod
    def fit(cls, X, y, n_trees=500, mtry=None, nodesize=5, inbag=None, seeds=None, seed=0, importance=False, n_perm=1,
            perm_seeds=None) -> "RandomForest":
        """randomForest::randomForest(mod.form, data = train) (V73:248 per CV fold, V73:517 the final model) with the
        package's regression defaults (ntree = 500, mtry = max(floor(p / 3), 1), nodesize = 5, bootstrap of n rows with
        replacement), grown on the device (mhs_rf_fit_many, a workgroup per tree).  ``inbag``: (n_trees, n) int32, how
        many times row i is in tree t's bootstrap; ``None`` draws n rows with replacement per tree from
        ``numpy.random.default_rng(seed)``.  ``seeds``: one uint64 per tree, driving the per-node variable draw;
        ``None`` draws them from the same generator (after the bags).  NOT R's RNG stream: the forest is randomForest's
        for these bags and draws, not for R's ``set.seed``; the random tie-break of recent randomForest releases is not
        reproduced (include/machisplin_hip.h).  ``importance = True`` (randomForest's ``importance = TRUE``, V73:517-519)
        runs :func:`rf_importance_many` on the fitted forest with ``n_perm`` permutations per tree and variable and the
        permutation seeds ``perm_seeds`` (``None``: a stream of their own, see there).  The object carries ``.params`` (the
        ``kind = "rf"`` dict of :func:`from_param_dict`), ``.oob_pred`` / ``.oob_count`` (the out-of-bag mean of every
        row, NaN where no tree left it out), ``.mse`` and ``.rsq`` (mean squared OOB error and
        ``1 - mse / mean((y - mean(y))^2)`` over the rows with ``oob_count > 0``), ``.inc_node_purity`` (IncNodePurity),
        ``.inbag`` and ``.seeds``."""
        return rf_fit_many([X], [y], n_trees, mtry, nodesize, None if inbag is None else [inbag],
                           None if seeds is None else [seeds], seed, importance, n_perm, None if perm_seeds is None else [perm_seeds])[0]

    def importance(self, X, y, inbag=None, perm_seeds=None, n_perm=1, seed=0) -> np.ndarray:
        """:func:`rf_importance_many` for this forest on its training rows: sets and returns ``.importance`` (which, an
        instance attribute from then on, stays callable with these arguments)."""
        rf_importance_many([self], [X], [y], None if inbag is None else [inbag], None if perm_seeds is None else [perm_seeds], n_perm, seed)
        return self.importance


def rf_fit_many(Xs, ys, n_trees=500, mtry=None, nodesize=5, inbag=None, seeds=None, seed=0, importance=False, n_perm=1,
                perm_seeds=None):
    """:meth:`RandomForest.fit` for several forests (each its own rows, bags and seeds; the same p, n_trees, mtry and
    nodesize) in ONE device call: the shape of the ten fold forests of V73:248.  ``inbag`` / ``seeds``: one array per
    model; ``seed``: an int (model k draws from ``default_rng([seed, k])``; a single model from ``default_rng(seed)``) or
    one per model.  ``importance``: one more device call, :func:`rf_importance_many` ``(models, Xs, ys, n_perm = n_perm,
    perm_seeds = perm_seeds, seed = seed)``, after the fit; the bags and the draw seeds are the same with and without it."""
    Xs, ys = _fit_inputs(Xs, ys)
    count, p, n_trees = len(Xs), Xs[0].shape[1], int(n_trees)
    mtry = max(p // 3, 1) if mtry is None else int(mtry)
    gen = _fit_generators(seed, count)
    bags, sds = [], []
    for k, X in enumerate(Xs):
        n = X.shape[0]
        rng = np.random.default_rng(gen[k]) if inbag is None or seeds is None else None
        if inbag is None:
            b = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(n_trees)])
        else:
            b = np.asarray(inbag[k])
            if b.shape != (n_trees, n):
                raise ValueError("inbag must be n_trees x n in-bag counts")
        if seeds is None:
            s = rng.integers(0, 2 ** 64, size=n_trees, dtype=np.uint64)
        else:
            s = np.asarray(seeds[k], dtype=np.uint64)
            if s.shape != (n_trees,):
                raise ValueError("seeds must hold one uint64 per tree")
        bags.append(_i32(b))
        sds.append(np.ascontiguousarray(s))
    hs = (C.c_void_p * count)()
    oobp = [np.empty(X.shape[0]) for X in Xs]
    oobc = [np.zeros(X.shape[0], dtype=np.int32) for X in Xs]
    pur = [np.empty(p) for _ in Xs]
    ns = _i64([X.shape[0] for X in Xs])
    _lib.init()
    _lib.check(_lib.lib().mhs_rf_fit_many(count, _ptrs(Xs), _ptrs(ys), ns.ctypes.data, p, n_trees, mtry, int(nodesize), _ptrs(bags),
                                          _ptrs(sds), hs, _ptrs(oobp), _ptrs(oobc), _ptrs(pur)))
    out = []
    for k in range(count):
        m = _adopt(RandomForest, hs[k], p)
        nn = C.c_int64()
        _lib.check(_lib.lib().mhs_rf_get(m._h, C.byref(nn), None, None, None, None, None, None, None))
        l, r, st, bv = (np.empty(nn.value, dtype=np.int32) for _ in range(4))
        sp, npred, off = np.empty(nn.value), np.empty(nn.value), np.empty(n_trees + 1, dtype=np.int64)
        _lib.check(_lib.lib().mhs_rf_get(m._h, C.byref(nn), l.ctypes.data, r.ctypes.data, st.ctypes.data, bv.ctypes.data,
                                         sp.ctypes.data, npred.ctypes.data, off.ctypes.data))
        m.params = {"kind": "rf", "tree_offsets": off, "left": l, "right": r, "status": st, "best_var": bv, "split": sp,
                    "node_pred": npred, "p": p}
        m.oob_pred, m.oob_count, m.inc_node_purity, m.inbag, m.seeds = oobp[k], oobc[k], pur[k], bags[k], sds[k]
        m.n_trees, m.mtry, m.nodesize = n_trees, mtry, int(nodesize)
        seen = oobc[k] > 0
        d = ys[k][seen] - oobp[k][seen]
        m.mse = float(np.mean(d * d)) if seen.any() else float("nan")
        dy = ys[k][seen] - np.mean(ys[k][seen]) if seen.any() else np.zeros(0)
        var = float(np.mean(dy * dy)) if seen.any() else 0.0
        m.rsq = 1.0 - m.mse / var if var > 0.0 else float("nan")
        out.append(m)
    if importance:
        rf_importance_many(out, Xs, ys, None, perm_seeds, n_perm, gen)
    return out


_IMPORTANCE_STREAM = 1 << 20       # the last word of the permutation seeds' stream: no fit stream [seed, k] ends in it (k < 65536)


def rf_importance_many(models, Xs, ys, inbag=None, perm_seeds=None, n_perm=1, seed=0):
    """randomForest's permutation importance (``importance = TRUE``: ``$importance[, "%IncMSE"]`` and ``$importanceSD``,
    what the reference stores as the forest's $var.imp, V73:517-519) of several forests -- any :class:`RandomForest`,
    loaded or fitted here; the same p and number of trees -- on their training rows, in ONE device call, a workgroup per
    tree (mhs_rf_importance_many; the rule is stated in include/machisplin_hip.h).  ``inbag``: one (n_trees, n) array of
    in-bag counts per model, as in the fit; ``None`` takes each model's ``.inbag`` (set when it was fitted here).
    ``perm_seeds``: one array of n_trees uint64 per model; ``None`` draws model k's from
    ``default_rng([*g_k, 2 ** 20])`` with ``g_k`` as :func:`_fit_generators` derives it from ``seed`` -- a stream of its
    own, NOT R's: the fit's bags and draw seeds are what they are without this call.  ``n_perm``: permutations per tree
    and variable (randomForest's ``nPerm``), 1 .. 16.

    Every model gains ``.importance`` (p x 2: the RAW ``%IncMSE`` as ``$importance`` holds it -- not divided by its SD --
    and ``IncNodePurity``, NaN for a forest that was not fitted here), ``.importance_sd`` (``$importanceSD``),
    ``.tree_delta`` (n_trees x p, every tree's increase) and ``.perm_seeds``.  Returns the models."""
    models = list(models)
    Xs, ys = _fit_inputs(Xs, ys)
    count, p = len(Xs), Xs[0].shape[1]
    if len(models) != count or any(not isinstance(m, RandomForest) for m in models):
        raise ValueError("need one RandomForest per predictor matrix")
    lib = _lib.lib()
    nt = C.c_int64()
    _lib.check(lib.mhs_model_info(models[0]._h, None, None, C.byref(nt)))
    n_trees = int(nt.value)
    if inbag is None:
        if any(getattr(m, "inbag", None) is None for m in models):
            raise ValueError("a forest that was not fitted here needs its inbag counts")
        inbag = [m.inbag for m in models]
    bags = [_i32(b) for b in inbag]
    if len(bags) != count or any(b.shape != (n_trees, X.shape[0]) for b, X in zip(bags, Xs)):
        raise ValueError("inbag must hold one n_trees x n array of in-bag counts per model")
    if perm_seeds is None:
        sds = [np.random.default_rng(np.atleast_1d(g).tolist() + [_IMPORTANCE_STREAM]).integers(0, 2 ** 64, size=n_trees, dtype=np.uint64)
               for g in _fit_generators(seed, count)]
    else:
        sds = [np.ascontiguousarray(np.asarray(s, dtype=np.uint64)) for s in perm_seeds]
        if len(sds) != count or any(s.shape != (n_trees,) for s in sds):
            raise ValueError("perm_seeds must hold one uint64 per tree and model")
    inc, sd = [np.empty(p) for _ in Xs], [np.empty(p) for _ in Xs]
    delta = [np.empty((n_trees, p)) for _ in Xs]
    ns = _i64([X.shape[0] for X in Xs])
    hs = (C.c_void_p * count)(*[m._h for m in models])
    _lib.check(lib.mhs_rf_importance_many(count, hs, _ptrs(Xs), _ptrs(ys), ns.ctypes.data, p, _ptrs(bags), _ptrs(sds), int(n_perm),
                                          _ptrs(inc), _ptrs(sd), _ptrs(delta)))
    for k, m in enumerate(models):
        pur = getattr(m, "inc_node_purity", None)
        m.importance = np.column_stack([inc[k], np.full(p, np.nan) if pur is None else pur]).view(_ImportanceTable)
        m.importance._model = weakref.ref(m)
        m.importance_sd, m.tree_delta, m.perm_seeds = sd[k], delta[k], sds[k]
    return models


def from_param_dict(m: dict) -> Model:
    """Build a device model from the plain parameter dict the tests and bench.py use
    (same fields as the flat R arrays; see the loaders in include/machisplin_hip.h)."""
    k = m["kind"]
    if k == "lm":
        return Gam(m["coef"])
    if k == "nnet":
        return Nnet(m["wts"], m["p"], m["size"], m["y_scale"], m["y_shift"])
    if k == "earth":
        return Earth(m["coef"], m["dirs"], m["cuts"])
    if k == "svr":
        return Ksvm(m["alpha"], m["sv"], m["b"], m["sigma"], m["x_center"], m["x_scale"], m["y_center"], m["y_scale"])
    if k == "gbm":
        return Gbm(m["init_f"], m["tree_offsets"], m["split_var"], m["split_val"], m["left"], m["right"],
                   m["missing"], m["p"])
    if k == "rf":
        return RandomForest(m["tree_offsets"], m["left"], m["right"], m["status"], m["best_var"], m["split"],
                            m["node_pred"], m["p"])
    raise ValueError(k)


def _window(stack: RasterStack, window):
    g = stack.geom
    return window if window is not None else (0, g.nrow, 0, g.ncol)


def _out(stack, window, out):
    import torch
    r0, r1, c0, c1 = window
    if out is None:
        out = torch.empty((r1 - r0, c1 - c0), dtype=torch.float64, device=stack.planes.device)
    if out.dtype != torch.float64 or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1 \
            or tuple(out.shape) != (r1 - r0, c1 - c0):
        raise ValueError("out must be a float64 device tensor of the window's shape with unit column stride")
    return out


def predict(stack: RasterStack, model: Model, window=None, weight: float = 1.0, accumulate: bool = False,
            out=None, stream=None):
    """terra::predict(rast_stack, model) over the whole raster or a window (r0, r1, c0, c1).
    ``out = pred * weight`` or, with accumulate, ``out += pred * weight`` (V73:471/475 ...)."""
    import torch
    if model.p != stack.n_layers + 2:
        raise ValueError("model expects p = layers + 2 predictors (covariates, LONG, LAT)")
    window = _window(stack, window)
    out = _out(stack, window, out)
    g, s = stack.geom.c_struct(), stack.c_struct()
    st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(_lib.lib().mhs_predict_dev(model._h, C.byref(g), C.byref(s), *window, float(weight),
                                          int(bool(accumulate)), out.data_ptr(), out.stride(0), st))
    return out


def ensemble_predict(stack: RasterStack, models, weights, wt_total: float, window=None, out=None, stream=None):
    """The Step-2 raster loop (V73:447-619): ``(((p1 w1) + p2 w2) + ...) / wt_total`` with the
    models in ``mods.run`` order, the rounded kept weights, and the UNROUNDED total."""
    import torch
    window = _window(stack, window)
    out = _out(stack, window, out)
    n = len(models)
    if n == 0 or n != len(weights):
        raise ValueError("need one weight per model")
    hs = (C.c_void_p * n)(*[m._h for m in models])
    ws = (C.c_double * n)(*[float(w) for w in weights])
    g, s = stack.geom.c_struct(), stack.c_struct()
    st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(_lib.lib().mhs_ensemble_predict_dev(hs, ws, n, float(wt_total), C.byref(g), C.byref(s), *window,
                                                   out.data_ptr(), out.stride(0), st))
    return out


def members_predict(stack: RasterStack, models, weights, window=None, accumulate: bool = False, out=None, stream=None):
    """``out (+)= sum_k w_k pred_k`` over the window, members in order: the accumulation lines of the Step-2 loop
    (V73:471 ... 605) without the final division.  Consecutive gam / nnet / earth members share one pass over the planes
    (bit-identical to calling :func:`predict` member by member)."""
    import torch
    window = _window(stack, window)
    out = _out(stack, window, out)
    n = len(models)
    if n == 0 or n != len(weights):
        raise ValueError("need one weight per model")
    hs = (C.c_void_p * n)(*[m._h for m in models])
    ws = (C.c_double * n)(*[float(w) for w in weights])
    g, s = stack.geom.c_struct(), stack.c_struct()
    st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(_lib.lib().mhs_members_predict_dev(hs, ws, n, C.byref(g), C.byref(s), *window, int(bool(accumulate)),
                                                  out.data_ptr(), out.stride(0), st))
    return out


def fit_reserve_cus(n_cus: int) -> int:
    """mhs_fit_reserve_cus: while n_cus > 0 the first tree / ksvm member of every ensemble call on a large window
    leaves n_cus compute units free for a concurrent Tps fit (results unchanged).  Returns the previous setting."""
    _lib.init()
    prev = C.c_int(0)
    _lib.check(_lib.lib().mhs_fit_reserve_cus(int(n_cus), C.byref(prev)))
    return int(prev.value)


def select_weights(p_opt, labels="bgnmrv"):
    """V73:336-362 / 375-392: keep model k iff round(p_k, 2) > 0.05 * sum(p); the kept
    weight is round(p_k, 2); the divisor stays the unrounded sum over ALL candidates."""
    p_opt = np.asarray(p_opt, dtype=np.float64)
    tot = float(p_opt.sum())
    kept, wts = "", []
    for lab, pk in zip(labels, p_opt):
        r = float(np.round(pk, 2))
        if r > 0.05 * tot:
            kept += lab
            wts.append(r)
    return kept, wts, tot
