"""Reference for the device growth of gbm's boosted trees (mhs_gbm_grow_many): a numpy restatement of gbm 2.x's
CART for distribution = "gaussian" (no weights, no offset, train.fraction = 1) with the bag of every tree given.

Not a port of any source: the rule as published --

* ``init_f = mean(y)``; per tree ``z = y - F``; the tree is grown on the bag rows;
* best-first: up to ``depth`` times, every terminal node's best split over variables 0 .. p-1 in that order, walking
  the node's bag rows in ascending order of the variable (stable: ties in row order); a candidate lies between
  consecutive distinct values with at least ``minobs`` bag rows on both sides, at ``0.5 * (x_prev + x)``, with
  improvement ``nL nR / (nL + nR) (meanL - meanR)^2``; only a strictly greater improvement replaces the best; the
  terminal node with the strictly greatest improvement, in terminal-list order (the left child takes its parent's
  slot, right and missing are appended), is split; growth stops when that improvement is 0;
* a split makes a left (``x < split``), a right and a missing child (the parent's mean: no NA in training rows);
* terminal values are ``shrinkage * mean(z over the node's bag rows)``; ``F += value`` for every row;
* nodes are stored in preorder: node, left, right, missing.

The left sums are accumulated SEQUENTIALLY along the sorted order (``np.cumsum``), in float64 or -- ``acc =
np.longdouble`` -- in extended precision.  An input on which both give the same structures is one whose structure
does not hinge on the summation order; only on such inputs is an exact structural comparison with the device (which
adds 64 rows at a time) a fair one."""
import numpy as np


def sort_orders(X):
    return [np.argsort(X[:, v], kind="stable") for v in range(X.shape[1])]


def _improvements(x, zc, tot, m, minobs):
    """improvement of every position j = 1 .. m-1 (0 where no candidate lies) for sorted values x, running sums zc"""
    j = np.arange(1, m)
    ok = (x[:-1] < x[1:]) & (j >= minobs) & (m - j >= minobs)
    ls = zc[:-1]
    nl = j.astype(zc.dtype)
    nr = (m - j).astype(zc.dtype)
    d = ls / nl - (tot - ls) / nr
    imp = nl * nr / (nl + nr) * d * d
    return np.where(ok, imp, 0), ls


def _best_split(X, z, segs, tot, minobs, acc, scan=np.cumsum, var_tie_last=False, pos_tie_high=False):
    m = segs[0].size
    best = (acc(0), -1, 0, 0.0, acc(0))         # imp, var, nL, split, left sum
    if m < 2:
        return best
    for v, r in enumerate(segs):
        x = X[r, v]
        zc = scan(z[r].astype(acc))
        imp, ls = _improvements(x, zc, tot, m, minobs)
        k = int(np.argmax(imp))                 # the first of equal maxima: the lowest position
        if pos_tie_high:
            k = imp.size - 1 - int(np.argmax(imp[::-1]))
        if imp[k] > best[0] or (var_tie_last and imp[k] == best[0] and imp[k] > 0):
            best = (imp[k], v, k + 1, 0.5 * (x[k] + x[k + 1]), ls[k])
    return best


def candidate_improvement(X, z, tree, node, var, split, minobs=10, acc=np.float64):
    """The improvement this reference computes for splitting creation-order node ``node`` of ``tree`` at (var, split)."""
    r = tree["segs"][node][var]
    m = r.size
    if m < 2:
        return 0.0
    x = X[r, var]
    zc = np.cumsum(z[r].astype(acc))
    imp, _ = _improvements(x, zc, tree["tot"][node], m, minobs)
    nl = int(np.searchsorted(x, split, side="left"))
    if nl < 1 or nl >= m:
        return 0.0
    return float(imp[nl - 1])


def grow_tree(X, z, bag, orders, depth=25, minobs=10, shrinkage=0.01, acc=np.float64, scan=np.cumsum, var_tie_last=False,
              pos_tie_high=False, node_tie_later=False):
    """One tree.  Returns a dict: the preorder arrays (split_var, split_val, left, right, missing), ``imp`` (the
    improvement of every internal node, preorder), ``pre`` (creation index -> preorder index), and per creation-order
    node ``segs`` (its bag rows in every variable's order) and ``tot``.  ``scan`` forms the running sums of z along a
    sorted order in place of np.cumsum.  The last three arguments grow DELIBERATELY WRONG trees, for the tests that show
    what an exact comparison catches (test_tree_ties_host.py): ``var_tie_last`` lets an equal improvement of a later
    variable replace the best ('>=' for '>'), ``pos_tie_high`` takes the highest position among equal improvements of
    one variable, ``node_tie_later`` splits the later of two terminal nodes with equal improvements."""
    search = lambda s, t_: _best_split(X, z, s, t_, minobs, acc, scan, var_tie_last, pos_tie_high)
    n, p = X.shape
    inbag = np.zeros(n, dtype=bool)
    inbag[bag] = True
    segs0 = [o[inbag[o]] for o in orders]
    tot0 = scan(z[segs0[0]].astype(acc))[-1]
    var, val, left, right, miss, imps = [-1], [tot0 / acc(segs0[0].size)], [-1], [-1], [-1], [0.0]
    segs, tot = [segs0], [tot0]
    term = [0]                                   # terminal list: creation indices
    best = {0: search(segs0, tot0)}
    empty = [np.zeros(0, dtype=np.int64)] * p
    for _ in range(depth):
        k, top = -1, acc(0)
        for slot, nd in enumerate(term):
            if best[nd][0] > top or (node_tie_later and best[nd][0] == top and top > 0):
                top, k = best[nd][0], slot
        if k < 0:
            break
        nd = term[k]
        imp, v, nl, sv, ls = best[nd]
        goes_left = np.zeros(n, dtype=bool)
        goes_left[segs[nd][v][:nl]] = True
        m = segs[nd][0].size
        nn = len(var)
        var[nd], left[nd], right[nd], miss[nd], imps[nd] = v, nn, nn + 1, nn + 2, float(imp)
        parent_mean = val[nd]
        val[nd] = sv
        sl = [r[goes_left[r]] for r in segs[nd]]
        sr = [r[~goes_left[r]] for r in segs[nd]]
        tl, tr = ls, tot[nd] - ls
        for s, t_, mean in ((sl, tl, tl / acc(nl)), (sr, tr, tr / acc(m - nl)), (empty, acc(0), parent_mean)):
            var.append(-1); val.append(mean); left.append(-1); right.append(-1); miss.append(-1); imps.append(0.0)
            segs.append(s); tot.append(t_)
        best[nn] = search(sl, tl)
        best[nn + 1] = search(sr, tr)
        best[nn + 2] = (acc(0), -1, 0, 0.0, acc(0))
        term[k] = nn
        term += [nn + 1, nn + 2]
    # preorder: node, left, right, missing
    pre, stack = {}, [0]
    while stack:
        e = stack.pop()
        pre[e] = len(pre)
        if var[e] >= 0:
            stack += [miss[e], right[e], left[e]]
    nn = len(var)
    out = {"split_var": np.full(nn, -1, dtype=np.int32), "split_val": np.zeros(nn), "left": np.full(nn, -1, dtype=np.int32),
           "right": np.full(nn, -1, dtype=np.int32), "missing": np.full(nn, -1, dtype=np.int32), "imp": np.zeros(nn),
           "pre": pre, "segs": segs, "tot": tot}
    for e in range(nn):
        o = pre[e]
        out["split_var"][o] = var[e]
        if var[e] >= 0:
            out["split_val"][o] = val[e]
            out["left"][o], out["right"][o], out["missing"][o] = pre[left[e]], pre[right[e]], pre[miss[e]]
            out["imp"][o] = imps[e]
        else:
            out["split_val"][o] = shrinkage * float(val[e])
    return out


def tree_values(tree, X):
    """The terminal value of every row of X (no NA)."""
    node = np.zeros(X.shape[0], dtype=np.int64)
    rows = np.arange(X.shape[0])
    while True:
        v = tree["split_var"][node]
        act = v >= 0
        if not act.any():
            return tree["split_val"][node]
        a = rows[act]
        na = node[act]
        node[act] = np.where(X[a, v[act]] < tree["split_val"][na], tree["left"][na], tree["right"][na])


def fit(X, y, n_trees, bags, depth=25, minobs=10, shrinkage=0.01, acc=np.float64, F=None, keep=False):
    """n_trees trees from F (None: from mean(y)).  Returns (params, F, trees): ``params`` is the kind = "gbm" bundle of
    the evaluators, ``trees`` the grow_tree dicts (segments dropped unless ``keep``)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    orders = sort_orders(X)
    init_f = float(np.mean(y))
    F = np.full(y.size, init_f) if F is None else np.array(F, dtype=np.float64)
    trees, off = [], [0]
    for t in range(n_trees):
        tr = grow_tree(X, y - F, np.asarray(bags[t]), orders, depth, minobs, shrinkage, acc)
        F = F + tree_values(tr, X)
        if not keep:
            tr.pop("segs"); tr.pop("tot")
        trees.append(tr)
        off.append(off[-1] + tr["split_var"].size)
    cat = lambda k: np.concatenate([t_[k] for t_ in trees])
    params = {"kind": "gbm", "init_f": init_f, "tree_offsets": np.array(off, dtype=np.int64), "split_var": cat("split_var"),
              "split_val": cat("split_val"), "left": cat("left"), "right": cat("right"), "missing": cat("missing"),
              "p": X.shape[1]}
    return params, F, trees


def same_structure(a, b):
    """Two trees (dicts with the preorder arrays) have equal split variables, bit-equal split values and topology."""
    if a["split_var"].size != b["split_var"].size or not np.array_equal(a["split_var"], b["split_var"]):
        return False
    s = a["split_var"] >= 0
    return (np.array_equal(a["split_val"][s], b["split_val"][s]) and np.array_equal(a["left"][s], b["left"][s])
            and np.array_equal(a["right"][s], b["right"][s]) and np.array_equal(a["missing"][s], b["missing"][s]))


def tree_of(params, t):
    """Tree t of a kind = "gbm" bundle as a dict of preorder arrays."""
    o0, o1 = int(params["tree_offsets"][t]), int(params["tree_offsets"][t + 1])
    return {k: np.asarray(params[k])[o0:o1] for k in ("split_var", "split_val", "left", "right", "missing")}


def near_tie(X, z, ref_tree, dev_tree, minobs=10, rel=1e-9):
    """For a reference tree (grow_tree with its segments kept) and a device tree that differ: True when, at the first
    differing node in preorder, the reference's own improvements of the two candidates agree to ``rel`` relative.
    Both split the node differently: the two (variable, value) candidates on that node's rows.  The device splits a
    node the reference left terminal: that candidate against the smallest improvement the reference accepted (the
    split its depth budget went to instead).  Anything else is not a tie."""
    inv = {o: e for e, o in ref_tree["pre"].items()}
    n_ref, n_dev = ref_tree["split_var"].size, dev_tree["split_var"].size
    for o in range(min(n_ref, n_dev)):
        rv, dv = int(ref_tree["split_var"][o]), int(dev_tree["split_var"][o])
        if rv == dv and (rv < 0 or ref_tree["split_val"][o] == dev_tree["split_val"][o]):
            continue
        e = inv[o]
        accepted = ref_tree["imp"][ref_tree["split_var"] >= 0]
        if rv >= 0 and dv >= 0:
            a = float(ref_tree["imp"][o])
            b = candidate_improvement(X, z, ref_tree, e, dv, float(dev_tree["split_val"][o]), minobs)
        elif dv >= 0:
            a = float(accepted.min()) if accepted.size else 0.0
            b = candidate_improvement(X, z, ref_tree, e, dv, float(dev_tree["split_val"][o]), minobs)
        else:
            return False        # the reference splits a node the device left terminal: not attributed to a tie
        return abs(a - b) <= rel * max(abs(a), abs(b))
    return False
