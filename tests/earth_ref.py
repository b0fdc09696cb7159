"""Reference for the device fit of earth (MARS) models (mhs_earth_fit_many): a numpy restatement of the rule that
include/machisplin_hip.h states above mhs_earth_fit_many.  Not a port of any source.

earth as the reference's call drives it: degree 1, backward pruning, penalty 2, thresh 0.001,
nk = min(200, max(20, 2 p)) + 1, automatic minspan / endspan, numeric predictors, no weights.  RSS0 = sum (y - mean y)^2.

* term 0 is the intercept; ``minspan = max(1, int(-log2(-(1 / (p n)) ln(1 - 0.05)) / 2.5))``,
  ``endspan = max(1, int(3 - log2(0.05 / p)))``, a positive argument overrides;
* eligible knots of variable v: rows in ascending stable order of x_v, positions ``endspan, endspan + minspan, ... <
  n - endspan``; a position j is eligible only if ``xs[j] > xs[j-1]`` (skipped otherwise, not shifted); the cut is xs[j];
* a forward step: Q an orthonormal basis of the current terms, r = y - QQ'y; per variable (a) the linear term when x_v
  is not in the span (``|x - QQ'x|^2 > 1e-10 |x|^2``), reduction ``(q_x . r)^2``; (b) per eligible knot the hinge
  ``h = max(0, x - t)`` orthogonalised against Q and q_x, admissible if the remainder's squared norm is ``> 1e-10 |h|^2``,
  reduction = the linear reduction (or 0) + ``(h_o . r')^2 / |h_o|^2``; a (b) candidate adds the pair ``max(0, x - t)``,
  ``max(0, t - x)`` when x_v was not yet in the span, the single hinge otherwise; candidates are ordered variables
  ascending, linear before knots, knots by position, and only a strictly greater reduction replaces the best;
* stopping, in this order: RSS0 == 0 ``constant``; nterms + 2 > nk ``nk``; best not > 0 ``none``; best / RSS0 < thresh
  ``thresh`` (not added); add; 1 - RSS / RSS0 > 1 - thresh ``rsq``; GRSq < -10 ``grsq``;
* ``GCV(k) = (RSS / n) / (1 - C / n)^2``, ``C = k + penalty (k - 1) / 2``, +inf when C >= n; GRSq = 1 - GCV / GCV(1);
* pruning: from the full forward basis repeatedly drop the non-intercept term whose removal raises the RSS least (lowest
  index on a tie); the selected size has the smallest GCV (the smaller size on a tie); coefficients are least squares on
  the selected terms.

:func:`fit` works by explicit orthogonalisation (every candidate's hinge is formed and projected) and brute-force least
squares per subset, in float64 or -- ``acc = np.longdouble`` -- extended precision.  The device works with prefix sums in
64-row steps, so its reductions differ from these in the last bits: the yardstick is the certificate :func:`check_model`,
which follows the DEVICE's choices and recomputes every candidate at every step.  A choice passes if it lies within the
tie window of the best candidate: relative 1e-9 of the step's best reduction plus 1e-12 RSS0.

A fitted record is a dict: ``forward`` (``dirs`` / ``cuts`` M x p in mhs_earth_load's layout, ``rss`` after the step that
added each term, ``stop``), ``selected`` (M bools), ``rss_per_subset`` / ``gcv_per_subset`` (M), ``prune_terms`` (M x M,
row k-1 = the forward indices kept at size k, padded with -1), ``coef`` / ``dirs`` / ``cuts`` of the selected terms in
forward order, ``rss``, ``gcv``, ``rsq``, ``grsq``."""
import math

import numpy as np

REL, ABS = 1e-9, 1e-12          # the tie window: REL * best + ABS * RSS0
SPAN_TOL = 1e-10


def default_nk(p):
    return min(200, max(20, 2 * p)) + 1


def spans(n, p, minspan=0, endspan=0):
    ms = max(1, int(-math.log2(-(1.0 / (p * n)) * math.log(1.0 - 0.05)) / 2.5))
    es = max(1, int(3.0 - math.log2(0.05 / p)))
    return (minspan if minspan > 0 else ms), (endspan if endspan > 0 else es)


def knot_positions(xs, minspan, endspan):
    """eligible 0-based positions in the sorted values xs"""
    pos = np.arange(endspan, xs.size - endspan, minspan)
    return pos[xs[pos] > xs[pos - 1]] if pos.size else pos


def gcv(rss, k, n, penalty):
    c = k + penalty * (k - 1) / 2.0
    return float("inf") if c >= n else (float(rss) / n) / (1.0 - c / n) ** 2


def column(X, term):
    v, d, t = term
    if v < 0:
        return np.ones(X.shape[0], dtype=X.dtype)
    if d == 2:
        return X[:, v].copy()
    return np.maximum(X[:, v] - t, 0) if d == 1 else np.maximum(t - X[:, v], 0)


def _orthonormal(cols, acc):
    """Gram-Schmidt, every column orthogonalised twice"""
    Q = np.empty((cols[0].size, len(cols)), dtype=acc)
    for k, c in enumerate(cols):
        q = c.astype(acc)
        for _ in range(2):
            if k:
                q = q - Q[:, :k] @ (Q[:, :k].T @ q)
        Q[:, k] = q / np.sqrt(q @ q)
    return Q


def _rss(cols, y, acc):
    """(RSS, coefficients) of least squares on the columns"""
    if acc is np.float64:
        B = np.column_stack(cols)
        beta = np.linalg.lstsq(B, y, rcond=None)[0]
        e = y - B @ beta
        return float(e @ e), beta
    Q = _orthonormal(cols, acc)
    e = y - Q @ (Q.T @ y)
    e = e - Q @ (Q.T @ e)
    B = np.column_stack(cols).astype(acc)
    R = Q.T @ B
    z = Q.T @ y
    beta = np.zeros(len(cols), dtype=acc)
    for k in range(len(cols) - 1, -1, -1):
        beta[k] = (z[k] - R[k, k + 1:] @ beta[k + 1:]) / R[k, k]
    return e @ e, beta


def candidates(X, Q, r, v):
    """The candidates of variable v in rule order: a list of (reduction, kind, cut); kind 2 linear, 1 pair, 3 single
    hinge."""
    acc = X.dtype.type
    x = X[:, v]
    out = []
    xo = x - Q @ (Q.T @ x)
    xo = xo - Q @ (Q.T @ xo)
    Q2, r2, lin = Q, r, acc(0)
    has_lin = bool(xo @ xo > SPAN_TOL * (x @ x))
    if has_lin:
        q = xo / np.sqrt(xo @ xo)
        lin = (q @ r) ** 2
        r2 = r - q * (q @ r)
        Q2 = np.column_stack([Q, q])
        out.append((lin, 2, 0.0))
    return out, x, Q2, r2, lin, has_lin


def _all_candidates(X, Q, r, minspan, endspan):
    """every candidate of a forward step in rule order: (reduction, v, kind, cut)"""
    out = []
    for v in range(X.shape[1]):
        lin_c, x, Q2, r2, lin, has_lin = candidates(X, Q, r, v)
        out += [(c[0], v, c[1], c[2]) for c in lin_c]
        xs = np.sort(x, kind="stable")
        pos = knot_positions(xs, minspan, endspan)
        if not pos.size:
            continue
        cuts = xs[pos]
        H = np.maximum(x[:, None] - cuts[None, :], 0)
        Ho = H - Q2 @ (Q2.T @ H)
        Ho = Ho - Q2 @ (Q2.T @ Ho)
        n2 = (Ho * Ho).sum(0)
        ok = n2 > SPAN_TOL * (H * H).sum(0)
        red = (Ho.T @ r2) ** 2 / np.where(ok, n2, 1)
        for t, rd, good in zip(cuts, red, ok):
            if good:
                out.append((lin + rd, v, 1 if has_lin else 3, float(t)))
    return out


def _best(cands):
    best = None
    for c in cands:
        if best is None or c[0] > best[0]:
            best = c
    return best


def _terms_of_step(v, kind, cut):
    if kind == 2:
        return [(v, 2, 0.0)]
    return [(v, 1, cut), (v, -1, cut)] if kind == 1 else [(v, 1, cut)]


def _dirs_cuts(terms, p):
    dirs = np.zeros((len(terms), p), dtype=np.int32)
    cuts = np.zeros((len(terms), p))
    for k, (v, d, t) in enumerate(terms):
        if v >= 0:
            dirs[k, v] = d
            cuts[k, v] = t
    return dirs, cuts


def terms_from(dirs, cuts):
    """the (variable, dir, cut) list of a dirs / cuts pair (the intercept is (-1, 0, 0))"""
    out = []
    for d, c in zip(np.asarray(dirs), np.asarray(cuts)):
        nz = np.flatnonzero(d)
        assert nz.size <= 1, "degree 1: at most one factor per term"
        out.append((int(nz[0]), int(d[nz[0]]), float(c[nz[0]])) if nz.size else (-1, 0, 0.0))
    return out


def steps_from(terms):
    """the forward steps of a term list: (v, kind, cut, number of terms)"""
    steps, k = [], 1
    while k < len(terms):
        v, d, t = terms[k]
        if d == 2:
            steps.append((v, 2, 0.0, 1))
        elif d == 1 and k + 1 < len(terms) and terms[k + 1] == (v, -1, t):
            steps.append((v, 1, t, 2))
        else:
            assert d == 1, "a lone hinge is max(0, x - t)"
            steps.append((v, 3, t, 1))
        k += steps[-1][3]
    return steps


def _stop_after_add(rss, rss0, nterms, n, thresh, penalty):
    """the rule's checks 6 and 7"""
    if 1.0 - float(rss) / float(rss0) > 1.0 - thresh:
        return "rsq"
    if 1.0 - gcv(rss, nterms, n, penalty) / gcv(rss0, 1, n, penalty) < -10.0:
        return "grsq"
    return None


def _prune(X, y, terms, acc):
    """backward pass by brute force: (rss_per_subset, prune_terms, window-decided steps)"""
    M = len(terms)
    cols = [column(X, t) for t in terms]
    rss0 = _rss(cols[:1], y, acc)[0]
    kept = list(range(M))
    rss_sub = np.zeros(M, dtype=acc)
    pt = -np.ones((M, M), dtype=np.int32)
    rss_sub[M - 1] = _rss(cols, y, acc)[0]
    pt[M - 1] = kept
    decided = 0
    for m in range(M, 1, -1):
        after = [_rss([cols[i] for i in kept if i != j], y, acc)[0] for j in kept[1:]]
        lo = int(np.argmin(after))                      # the first minimum: the lowest index on a tie
        win = REL * float(after[lo] - rss_sub[m - 1]) + ABS * float(rss0)
        decided += sum(1 for a in after if a <= after[lo] + win) > 1
        kept = [i for i in kept if i != kept[1 + lo]]
        rss_sub[m - 2] = after[lo]
        pt[m - 2, :m - 1] = kept
    return rss_sub, pt, decided


def fit(X, y, nk=None, thresh=0.001, penalty=2.0, minspan=0, endspan=0, acc=np.float64):
    """The rule in ``acc`` arithmetic; returns the record (plus ``window_decided``: the number of forward steps, pruning
    steps and GCV choices with a runner-up inside the tie window)."""
    Xd, yd = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = Xd.shape
    nk = default_nk(p) if nk is None or nk <= 0 else nk
    ms, es = spans(n, p, minspan, endspan)
    X, y = Xd.astype(acc), yd.astype(acc)
    terms, rss_f, decided = [(-1, 0, 0.0)], [], 0
    r = y - y.mean()
    rss0 = r @ r
    rss_f.append(rss0)
    rss = rss0
    stop = None
    if rss0 == 0:
        stop = "constant"
    while stop is None:
        if len(terms) + 2 > nk:
            stop = "nk"
            break
        Q = _orthonormal([column(X, t) for t in terms], acc)
        r = y - Q @ (Q.T @ y)
        r = r - Q @ (Q.T @ r)
        cands = _all_candidates(X, Q, r, ms, es)
        best = _best(cands)
        if best is None or not best[0] > 0:
            stop = "none"
            break
        win = REL * float(best[0]) + ABS * float(rss0)
        decided += sum(1 for c in cands if c[0] >= best[0] - win) > 1
        if best[0] / rss0 < thresh:
            stop = "thresh"
            break
        new = _terms_of_step(best[1], best[2], best[3])
        terms += new
        rss = _rss([column(X, t) for t in terms], y, acc)[0]
        rss_f += [rss] * len(new)
        stop = _stop_after_add(rss, rss0, len(terms), n, thresh, penalty)
    M = len(terms)
    rss_sub, pt, dec_p = _prune(X, y, terms, acc)
    decided += dec_p
    g = np.array([gcv(rss_sub[k - 1], k, n, penalty) for k in range(1, M + 1)])
    ksel = int(np.argmin(g)) + 1 if np.isfinite(g).any() else 1
    decided += int(np.sum(g <= g[ksel - 1] * (1.0 + REL)) > 1) if np.isfinite(g[ksel - 1]) else 0
    keep = [int(i) for i in pt[ksel - 1, :ksel]]
    sel_terms = [terms[i] for i in keep]
    _, beta = _rss([column(X, t) for t in sel_terms], y, acc)
    fd, fc = _dirs_cuts(terms, p)
    sd, sc = _dirs_cuts(sel_terms, p)
    selected = np.zeros(M, dtype=bool)
    selected[keep] = True
    g1 = gcv(rss0, 1, n, penalty)
    return {"forward": {"dirs": fd, "cuts": fc, "rss": np.array(rss_f, dtype=np.float64), "stop": stop},
            "selected": selected, "rss_per_subset": rss_sub.astype(np.float64), "gcv_per_subset": g, "prune_terms": pt,
            "coef": np.asarray(beta, dtype=np.float64), "dirs": sd, "cuts": sc, "rss": float(rss_sub[ksel - 1]),
            "gcv": float(g[ksel - 1]), "rsq": 1.0 - float(rss_sub[ksel - 1]) / float(rss0) if rss0 > 0 else 0.0,
            "grsq": 1.0 - float(g[ksel - 1]) / g1 if rss0 > 0 else 0.0, "window_decided": decided, "rss0": float(rss0)}


def same_structure(a, b):
    """two records made the same forward choices, pruned the same terms and selected the same size"""
    return (np.array_equal(a["forward"]["dirs"], b["forward"]["dirs"]) and np.array_equal(a["forward"]["cuts"], b["forward"]["cuts"])
            and a["forward"]["stop"] == b["forward"]["stop"] and np.array_equal(a["prune_terms"], b["prune_terms"])
            and np.array_equal(a["selected"], b["selected"]))


def check_model(X, y, rec, nk=None, thresh=0.001, penalty=2.0, minspan=0, endspan=0):
    """The certificate: follow the record's OWN forward choices step by step, recompute every candidate's reduction in
    float64 by explicit orthogonalisation, and assert that the choice lies within the tie window of the best candidate,
    that the recorded RSS matches (to the window) and that the stop reason is the rule's; the same for every pruning step
    (brute-force least squares per subset) and for the GCV choice.  Returns the number of steps decided inside the
    window (a runner-up other than the choice itself within the window of the best)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = X.shape
    nk = default_nk(p) if nk is None or nk <= 0 else nk
    ms, es = spans(n, p, minspan, endspan)
    fwd = rec["forward"]
    terms = terms_from(fwd["dirs"], fwd["cuts"])
    M = len(terms)
    assert terms[0] == (-1, 0, 0.0) and len(fwd["rss"]) == M
    r = y - y.mean()
    rss0 = float(r @ r)
    # (the last term is the rounding floor of a float64 residual, (16 eps)^2 |y|^2: all that is left when RSS0 == 0)
    tol = lambda v: REL * abs(float(v)) + ABS * rss0 + (16.0 * np.finfo(np.float64).eps) ** 2 * float(y @ y)
    assert abs(fwd["rss"][0] - rss0) <= tol(rss0), (fwd["rss"][0], rss0)
    decided = 0
    have = [terms[0]]
    stop = "constant" if rss0 == 0 else None
    steps = steps_from(terms)
    at = 0
    while stop is None:
        if len(have) + 2 > nk:
            stop = "nk"
            break
        Q = _orthonormal([column(X, t) for t in have], np.float64)
        r = y - Q @ (Q.T @ y)
        r = r - Q @ (Q.T @ r)
        cands = _all_candidates(X, Q, r, ms, es)
        best = _best(cands)
        more = at < len(steps)
        if best is None or not best[0] > tol(0.0):
            assert not more, "the record goes on where no candidate reduces the RSS"
            stop = "none"
            break
        win = tol(best[0])
        frac = best[0] / rss0
        if not more:
            # the record stopped here without adding: the rule's reason must be thresh (none is handled above)
            assert frac < thresh + win / rss0, ("the record stops where the rule goes on", frac)
            decided += frac >= thresh - win / rss0
            stop = "thresh"
            break
        v, kind, cut, cnt = steps[at]
        mine = [c for c in cands if c[1] == v and c[2] == kind and (kind == 2 or c[3] == cut)]
        assert len(mine) == 1, ("the step is no candidate of the rule", steps[at])
        assert mine[0][0] >= best[0] - win, ("step %d: reduction %r, the best candidate has %r" % (at, mine[0], best))
        decided += sum(1 for c in cands if c[0] >= best[0] - win) > 1
        assert frac >= thresh - win / rss0, ("the record goes on below thresh", frac)
        decided += frac < thresh + win / rss0
        have += _terms_of_step(v, kind, cut)
        rss = _rss([column(X, t) for t in have], y, np.float64)[0]
        for k in range(len(have) - cnt, len(have)):
            assert abs(fwd["rss"][k] - rss) <= tol(rss), ("forward RSS", k, fwd["rss"][k], rss)
        at += 1
        stop = _stop_after_add(rss, rss0, len(have), n, thresh, penalty)
        if stop is None and at == len(steps) and fwd["stop"] in ("rsq", "grsq"):
            raise AssertionError("the record stops with %s where the rule goes on" % fwd["stop"])
    assert at == len(steps) and len(have) == M, "the rule stops before the record does"
    assert fwd["stop"] == stop, (fwd["stop"], stop)
    # ---- pruning
    cols = [column(X, t) for t in terms]
    pt = np.asarray(rec["prune_terms"])
    rs = np.asarray(rec["rss_per_subset"], dtype=np.float64)
    assert pt.shape == (M, M) and rs.shape == (M,)
    assert list(pt[M - 1]) == list(range(M))
    full = _rss(cols, y, np.float64)[0]
    assert abs(rs[M - 1] - full) <= tol(full), (rs[M - 1], full)
    for m in range(M, 1, -1):
        kept = [int(i) for i in pt[m - 1, :m]]
        nxt = [int(i) for i in pt[m - 2, :m - 1]]
        assert np.all(pt[m - 1, m:] == -1) and kept[0] == 0
        gone = [i for i in kept if i not in nxt]
        assert len(gone) == 1 and gone[0] != 0 and nxt == [i for i in kept if i != gone[0]], ("not one term dropped", kept, nxt)
        before = _rss([cols[i] for i in kept], y, np.float64)[0]
        after = {j: _rss([cols[i] for i in kept if i != j], y, np.float64)[0] for j in kept[1:]}
        lo = min(after.values())
        win = REL * abs(lo - before) + ABS * rss0
        assert after[gone[0]] <= lo + win, ("size %d: dropped term %d raises the RSS to %r, the best to %r" % (m, gone[0], after[gone[0]], lo))
        decided += sum(1 for a in after.values() if a <= lo + win) > 1
        assert abs(rs[m - 2] - after[gone[0]]) <= tol(after[gone[0]]), ("RSS per subset", m - 1, rs[m - 2], after[gone[0]])
    # ---- the GCV choice, on the certified RSS per subset
    g = np.array([gcv(rs[k - 1], k, n, penalty) for k in range(1, M + 1)])
    gd = np.asarray(rec["gcv_per_subset"], dtype=np.float64)
    fin = np.isfinite(g)
    assert np.array_equal(fin, np.isfinite(gd)) and np.all(np.abs(gd[fin] - g[fin]) <= 1e-12 * np.abs(g[fin]))
    sel = np.asarray(rec["selected"]).astype(bool)
    ksel = int(sel.sum())
    assert sel[0] and sorted(np.flatnonzero(sel)) == sorted(int(i) for i in pt[ksel - 1, :ksel])
    if fin.any():
        lo = g[fin].min()
        assert g[ksel - 1] <= lo * (1.0 + REL), ("GCV choice", ksel, g)
        near = np.flatnonzero(fin & (g <= lo * (1.0 + REL)))
        decided += near.size > 1
        if near.size == 1 or np.all(g[near] == lo):
            assert ksel == int(np.flatnonzero(g == lo)[0]) + 1       # the smaller size on a tie
    else:
        assert ksel == 1
    keep = [int(i) for i in pt[ksel - 1, :ksel]]
    sd, sc = _dirs_cuts([terms[i] for i in keep], p)
    assert np.array_equal(rec["dirs"], sd) and np.array_equal(rec["cuts"], sc)
    assert abs(rec["rss"] - rs[ksel - 1]) <= tol(rs[ksel - 1]) and (not fin[ksel - 1] or abs(rec["gcv"] - g[ksel - 1]) <= 1e-12 * g[ksel - 1])
    if rss0 > 0:
        assert abs(rec["rsq"] - (1.0 - rs[ksel - 1] / rss0)) <= 1e-9
        g1 = gcv(rss0, 1, n, penalty)
        if fin[ksel - 1] and np.isfinite(g1):
            assert abs(rec["grsq"] - (1.0 - g[ksel - 1] / g1)) <= 1e-9
    return int(decided)


def basis(X, dirs, cuts):
    """the basis matrix of a dirs / cuts pair"""
    X = np.asarray(X, dtype=np.float64)
    return np.column_stack([column(X, t) for t in terms_from(dirs, cuts)])
