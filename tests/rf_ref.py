"""Reference for the device growth of randomForest's regression forests (mhs_rf_fit_many): a numpy restatement of the
growth rule with the randomness given -- per tree the in-bag counts of every row and one uint64 seed.

Not a port of any source: the rule as the header states it --

* ``mix(z)``: ``z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
  z ^ z >> 31`` (mod 2^64); the candidates of node k (0-based creation index) of a tree with seed s: ``ind = [0 .. p-1]``,
  ``last = p-1``; for j in 0 .. mtry-1: ``i = mix(mix(s + k) + j) mod (last + 1)``, take ``ind[i]``, ``ind[i] = ind[last]``,
  ``last -= 1``;
* a row with count c weighs c in every sum and every population count;
* nodes are numbered in creation order and processed in index order; splitting node k appends its left and then its
  right child; a non-root node of population <= nodesize is terminal, and so is a node with no admissible candidate;
* for each drawn variable, in draw order, the node's in-bag rows in ascending order of the variable (stable); a candidate
  lies between consecutive distinct values, criterion ``sl^2 / nl + sr^2 / nr - tot^2 / m``; only a strictly greater
  criterion replaces the best; a best that is not > 0 leaves the node terminal;
* split value ``0.5 (a + b)``, or ``a`` when that is not ``< b``; ``x <= split`` goes left; ``node_pred = tot / m``.

The sums are accumulated SEQUENTIALLY along the sorted order (``np.cumsum``), in float64 or -- ``acc = np.longdouble`` --
in extended precision.  With nodesize 5 the two disagree on the structure of nearly every tree (small nodes offer two
variables that cut off the same rows; their criteria differ only in the rounding of the sums), so the yardstick for the
device is not tree-versus-tree equality but the certificate walk :func:`check_tree`.

A tree is a dict of tree-local arrays in mhs_rf_load's layout: ``left`` / ``right`` (1-based, 0 at terminals),
``status`` (-3 / -1), ``best_var`` (1-based, 0 at terminals), ``split``, ``node_pred``."""
import numpy as np

_M = (1 << 64) - 1
KEYS = ("left", "right", "status", "best_var", "split", "node_pred")


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def draw_vars(seed, k, p, mtry):
    """The variables drawn for node k (0-based creation index) of a tree with seed ``seed``, in draw order."""
    ind, last, out = list(range(p)), p - 1, []
    h = mix((int(seed) + int(k)) & _M)
    for j in range(mtry):
        i = mix((h + j) & _M) % (last + 1)
        out.append(ind[i])
        ind[i] = ind[last]
        last -= 1
    return out


def _candidates(X, y, counts, rows, v, acc, scan=np.cumsum):
    """The candidates of a node (``rows`` ascending) along variable v: (criteria, a, b, rows left) per candidate, in
    position order, with sequential sums in ``acc`` (``scan``: what forms the running sums of c y in place of np.cumsum)."""
    o = np.argsort(X[rows, v], kind="stable")
    r = rows[o]
    x = X[r, v]
    c = counts[r]
    wc = scan((c * y[r]).astype(acc))
    cc = np.cumsum(c)
    tot, m = wc[-1], acc(cc[-1])
    at = np.flatnonzero(x[:-1] < x[1:])
    sl, nl = wc[at], cc[at].astype(acc)
    sr, nr = tot - sl, m - nl
    crit = sl * sl / nl + sr * sr / nr - tot * tot / m
    return crit, x[at], x[at + 1], at + 1, r


def split_value(a, b):
    mid = 0.5 * (a + b)
    return mid if mid < b else a


def grow_tree(X, y, counts, seed, mtry, nodesize=5, acc=np.float64, scan=np.cumsum, var_tie_last=False, pos_tie_high=False):
    """One tree.  Returns the dict of tree-local arrays plus ``rows`` (the in-bag rows of every node).  ``scan`` forms the
    running sums of c y along a sorted order in place of np.cumsum.  The last two arguments grow DELIBERATELY WRONG trees,
    for the tests that show what an exact comparison catches (test_tree_ties_host.py): ``var_tie_last`` lets an equal
    criterion of a later drawn variable replace the best ('>=' for '>'), ``pos_tie_high`` takes the highest position
    among equal criteria of one variable."""
    counts = np.asarray(counts, dtype=np.int64)
    p = X.shape[1]
    rows = [np.flatnonzero(counts > 0)]
    left, right, var, split, pred = [0], [0], [0], [0.0], []
    k = 0
    while k < len(rows):
        rk = rows[k]
        c = counts[rk]
        m = int(c.sum())
        pred.append(float(scan((c * y[rk]).astype(acc))[-1] / acc(m)))
        if (k == 0 or m > nodesize) and rk.size >= 2:
            best = (acc(0), -1, 0.0, None)
            for v in draw_vars(seed, k, p, mtry):
                crit, a, b, nl, r = _candidates(X, y, counts, rk, v, acc, scan)
                if crit.size:
                    j = int(np.argmax(crit))            # the first of equal maxima: the lowest position
                    if pos_tie_high:
                        j = crit.size - 1 - int(np.argmax(crit[::-1]))
                    if crit[j] > best[0] or (var_tie_last and crit[j] == best[0] and crit[j] > 0):
                        best = (crit[j], v, split_value(a[j], b[j]), r[:nl[j]])
            if best[1] >= 0:
                go_left = np.zeros(X.shape[0], dtype=bool)
                go_left[best[3]] = True
                nn = len(rows)
                left[k], right[k], var[k], split[k] = nn + 1, nn + 2, best[1] + 1, float(best[2])
                rows += [rk[go_left[rk]], rk[~go_left[rk]]]
                left += [0, 0]; right += [0, 0]; var += [0, 0]; split += [0.0, 0.0]
        k += 1
    left = np.array(left, dtype=np.int32)
    return {"left": left, "right": np.array(right, dtype=np.int32), "status": np.where(left > 0, -3, -1).astype(np.int32),
            "best_var": np.array(var, dtype=np.int32), "split": np.array(split), "node_pred": np.array(pred), "rows": rows}


def terminal_nodes(tree, X):
    """The (0-based) terminal node every row of X lands in: x <= split goes left."""
    node = np.zeros(X.shape[0], dtype=np.int64)
    rows = np.arange(X.shape[0])
    while True:
        act = tree["status"][node] != -1
        if not act.any():
            return node
        a, na = rows[act], node[act]
        node[act] = np.where(X[a, tree["best_var"][na] - 1] <= tree["split"][na], tree["left"][na], tree["right"][na]) - 1


def predict(tree, X):
    """The tree's prediction for every row of X."""
    return tree["node_pred"][terminal_nodes(tree, X)]


def tree_of(params, t):
    """Tree t of a kind = "rf" bundle as a dict of tree-local arrays."""
    o0, o1 = int(params["tree_offsets"][t]), int(params["tree_offsets"][t + 1])
    return {k: np.asarray(params[k])[o0:o1] for k in KEYS}


def bundle(trees, p):
    """The kind = "rf" bundle of the evaluators from a list of trees."""
    out = {k: np.concatenate([t[k] for t in trees]) for k in KEYS}
    out.update(kind="rf", p=p, tree_offsets=np.concatenate([[0], np.cumsum([t["left"].size for t in trees])]).astype(np.int64))
    return out


def oob(trees, X, inbag):
    """(oob_pred, oob_count): the mean, in tree order, of the predictions of the trees with inbag == 0 for the row."""
    s, w = np.zeros(X.shape[0]), np.zeros(X.shape[0], dtype=np.int32)
    for t, tr in enumerate(trees):
        out = np.asarray(inbag[t]) == 0
        s[out] = s[out] + predict(tr, X[out])
        w[out] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w > 0, s / w, np.nan), w


def check_tree(X, y, counts, seed, mtry, nodesize, tree, acc=np.float64, rel=1e-9):
    """The certificate walk: every node of ``tree`` (e.g. the device's) against the growth rule on its own in-bag rows.
    Raises AssertionError at the first violation; returns a dict: ``nodes`` (the node count), ``near_ties`` (how many
    internal nodes were NOT decided by a clear winner of the reference's criteria; they are still held to
    near-optimality), ``internal`` (the internal nodes), ``leaf`` (the terminal node of every in-bag row, -1 for the
    others) and ``crit`` (per node, the reference's criterion of the tree's split, 0 at terminals)."""
    counts = np.asarray(counts, dtype=np.int64)
    left, right, status, bvar, split, pred = (np.asarray(tree[k]) for k in KEYS)
    nn, p = left.size, X.shape[1]
    assert nn >= 1 and all(np.asarray(tree[k]).size == nn for k in KEYS)
    tol = 1e-12 * np.abs(y).max()
    rows = {0: np.flatnonzero(counts > 0)}
    leaf = np.full(X.shape[0], -1, dtype=np.int64)
    free, ties = 1, 0
    crits = np.zeros(nn)
    for k in range(nn):
        assert k in rows, "node %d is nobody's child" % k
        rk = rows.pop(k)
        c = counts[rk]
        m = int(c.sum())
        mean = float(np.sum((c * y[rk]).astype(np.longdouble)) / m)
        assert abs(pred[k] - mean) <= tol, "node %d: node_pred %r, weighted mean %r" % (k, pred[k], mean)
        cand = []
        if rk.size >= 2:
            drawn = draw_vars(seed, k, p, mtry)
            cand = [(v,) + _candidates(X, y, counts, rk, v, acc)[:4] for v in drawn]
        if status[k] == -1:
            assert left[k] == 0 and right[k] == 0 and bvar[k] == 0, "terminal node %d carries daughters or a variable" % k
            if not (k > 0 and m <= nodesize):
                floor = rel * float(np.sum(c * y[rk] * y[rk]))
                top = max([float(cr.max()) for _, cr, _, _, _ in cand if cr.size], default=0.0)
                assert top <= floor, "node %d is terminal but a candidate has criterion %r" % (k, top)
            leaf[rk] = k
            continue
        assert status[k] == -3, "node %d: status %d" % (k, status[k])
        assert left[k] == free + 1 and right[k] == free + 2, "node %d: daughters %d, %d, next free %d" % (k, left[k], right[k], free + 1)
        assert right[k] <= nn
        free += 2
        assert k == 0 or m > nodesize, "node %d of population %d was split (nodesize %d)" % (k, m, nodesize)
        v = int(bvar[k]) - 1
        assert v in drawn, "node %d: variable %d is not among the drawn %r" % (k, v, drawn)
        _, crit, a, b, _ = cand[drawn.index(v)]
        expect = np.where(0.5 * (a + b) < b, 0.5 * (a + b), a)
        hit = np.flatnonzero(expect == split[k])
        assert hit.size == 1, "node %d: split %r is no midpoint of consecutive distinct values" % (k, split[k])
        mine = crits[k] = float(crit[hit[0]])
        allc = np.concatenate([cr for _, cr, _, _, _ in cand])
        best = float(allc.max())
        assert mine >= (1 - rel) * best and mine > 0, "node %d: criterion %r, the best is %r" % (k, mine, best)
        second = float(np.partition(allc, -2)[-2]) if allc.size > 1 else -np.inf
        if best - second > rel * best:              # a clear winner: exactly that (variable, split); first maximum in draw order
            j = int(np.argmax(allc))
            for vv, cr, aa, bb, _ in cand:
                if j < cr.size:
                    assert vv == v and split_value(aa[j], bb[j]) == split[k], "node %d: the clear winner is (%d, %r), the tree has (%d, %r)" % (
                        k, vv, split_value(aa[j], bb[j]), v, split[k])
                    break
                j -= cr.size
        else:
            ties += 1
        go = X[rk, v] <= split[k]
        rows[int(left[k]) - 1], rows[int(right[k]) - 1] = rk[go], rk[~go]
        assert go.any() and not go.all()
    assert free == nn and not rows, "the tree has %d nodes, the numbering accounts for %d" % (nn, free)
    return {"nodes": nn, "near_ties": ties, "internal": int(np.sum(status == -3)), "leaf": leaf, "crit": crits}
