"""numpy restatements of the flow-path rule (include/machisplin_hip.h, section "flow paths"), independent of the library.

Two of them: :func:`walk` follows every cell's path step by step, :func:`doubling` is Jacobi pointer doubling over the whole
plane with numpy gathers (and counts its rounds, which ``info["rounds"]`` of the library must equal without the local phase).
Both return (end, n_ew, n_ns, n_d) as int64 planes, ``end`` the cell number of the stop cell the path reaches;
:func:`products` makes every plane and count of the rule from them.  Also the planes the tests run on.
"""
import numpy as np

import hydro_ref as hr
import proximity_ref as pr

WHERE = pr.WHERE + ("outlet",)
MAX_ROUNDS = 32


class Malformed(ValueError):
    pass


class Cycle(ValueError):
    pass


def seed(flowdir, target):
    """(ptr, n_ew, n_ns, n_d) of every cell as int64 planes: roots, targets and NA cells point at themselves with counts 0, every
    other cell at next() with the one step counted.  Malformed: a code outside -2 .. 7, a pointer out of the raster or at NA."""
    d = np.asarray(flowdir).astype(np.int64)
    nrow, ncol = d.shape
    r, c = np.meshgrid(np.arange(nrow, dtype=np.int64), np.arange(ncol, dtype=np.int64), indexing="ij")
    if ((d < -2) | (d > 7)).any():
        raise Malformed("code")
    flows = d >= 0
    k = np.where(flows, d, 0)
    rr, cc = r + np.asarray(hr.K_DR)[k], c + np.asarray(hr.K_DC)[k]
    inside = (rr >= 0) & (rr < nrow) & (cc >= 0) & (cc < ncol)
    if (flows & ~inside).any():
        raise Malformed("out of the raster")
    if (flows & (d[np.where(inside, rr, 0), np.where(inside, cc, 0)] == hr.DIR_NA)).any():
        raise Malformed("at an NA cell")
    moves = flows & ~np.asarray(target, dtype=bool)
    ptr = np.where(moves, rr * ncol + cc, r * ncol + c)
    ew = (moves & ((k == 0) | (k == 4))).astype(np.int64)
    ns = (moves & ((k == 2) | (k == 6))).astype(np.int64)
    dg = (moves & (k % 2 == 1)).astype(np.int64)
    return ptr, ew, ns, dg


def walk(flowdir, target):
    """every cell's path followed step by step, down to the first cell whose answer is known already; the answers of the cells
    passed are then filled in on the way back up"""
    ptr, ew, ns, dg = (a.ravel().tolist() for a in seed(flowdir, target))
    n = len(ptr)
    end = [-1] * n
    cnt = np.zeros((3, n), dtype=np.int64)
    for c in range(n):
        path, p = [], c
        while end[p] < 0 and ptr[p] != p:
            path.append(p)
            p = ptr[p]
            if len(path) > n:
                raise Cycle()
        if end[p] < 0:
            end[p] = p                                       # a stop cell
        for q in reversed(path):
            nxt = ptr[q]
            end[q] = end[nxt]
            cnt[0, q] = cnt[0, nxt] + ew[q]; cnt[1, q] = cnt[1, nxt] + ns[q]; cnt[2, q] = cnt[2, nxt] + dg[q]
    end = np.array(end, dtype=np.int64)
    shape = np.asarray(flowdir).shape
    return end.reshape(shape), cnt[0].reshape(shape), cnt[1].reshape(shape), cnt[2].reshape(shape)


def doubling(flowdir, target, rounds_out=None):
    """Jacobi pointer doubling: every round reads the records as they stood before it.  rounds_out: a list that receives the
    number of rounds in which a cell moved."""
    shape = np.asarray(flowdir).shape
    ptr, ew, ns, dg = (a.ravel().copy() for a in seed(flowdir, target))
    self = np.arange(ptr.size, dtype=np.int64)
    rounds = 0
    for launch in range(MAX_ROUNDS):
        pp = ptr[ptr]
        move = (ptr != self) & (pp != ptr)
        if (move & (pp == self)).any():                      # no forest has this: a cycle of 2^k cells would fold into self-pointers
            raise Cycle()
        if not move.any():
            break
        ew, ns, dg = ew + np.where(move, ew[ptr], 0), ns + np.where(move, ns[ptr], 0), dg + np.where(move, dg[ptr], 0)
        ptr = np.where(move, pp, ptr)
        rounds += 1
    else:
        raise Cycle()
    if rounds_out is not None:
        rounds_out.append(rounds)
    return ptr.reshape(shape), ew.reshape(shape), ns.reshape(shape), dg.reshape(shape)


def targets(flowdir, z, nodata, where, threshold=None):
    """the boolean target plane: valid cells whose layer value satisfies `where`; none for "outlet" """
    d = np.asarray(flowdir)
    if where == "outlet":
        return np.zeros(d.shape, dtype=bool)
    return pr.features(z, nodata, where, threshold) & (d != hr.DIR_NA)


def _na(v, nodata):
    v = np.asarray(v).astype(np.float64)
    na = np.isnan(v)
    if nodata is not None and not np.isnan(nodata):
        na |= v == nodata
    return np.where(na, np.nan, v)


def products(flowdir, target, root_ok, search_result, dx=1.0, dy=1.0, value_plane=None, nodata=None, f32=False):
    """the five planes of the rule and the info counts from (end, n_ew, n_ns, n_d): (dict of planes, dict of counts)"""
    d = np.asarray(flowdir)
    end, ew, ns, dg = search_result
    valid = d != hr.DIR_NA
    reached = valid & (root_ok | np.asarray(target, dtype=bool).ravel()[end])
    steps = ew + ns + dg
    g = np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy))
    dist = (ew.astype(np.float64) * np.float64(dx) + ns.astype(np.float64) * np.float64(dy)) + dg.astype(np.float64) * g
    out = {"index": np.where(reached, end, -1).astype(np.int32), "steps": np.where(reached, steps, -1).astype(np.int32)}
    flo = {"dist": dist}
    if value_plane is not None:
        v = _na(value_plane, nodata)
        flo["value"] = v.ravel()[end]
        flo["drop"] = v - v.ravel()[end]
    for k, a in flo.items():
        a = np.where(reached, a, np.nan)
        out[k] = a.astype(np.float32) if f32 else a
    info = {"n_valid": int(valid.sum()), "n_targets": int((np.asarray(target, dtype=bool) & valid).sum()), "n_roots": int((d == hr.DIR_OUT).sum()),
            "n_unreached": int((valid & ~reached).sum()), "max_steps": int(steps[reached].max()) if reached.any() else -1}
    return out, info


def flowpath(flowdir, z=None, nodata=None, where="outlet", threshold=None, root_is_target=True, dx=1.0, dy=1.0, value_plane=None, f32=False,
             search=doubling):
    """every plane of the rule: (planes, info); info has "rounds" when the search is :func:`doubling` """
    t = targets(flowdir, z, nodata, where, threshold)
    rounds = []
    res = search(flowdir, t, rounds) if search is doubling else search(flowdir, t)
    out, info = products(flowdir, t, bool(root_is_target) or where == "outlet", res, dx, dy, value_plane, nodata, f32)
    if rounds:
        info["rounds"] = rounds[0]
    return out, info


# ---- the planes of the tests ---------------------------------------------------------------------------------------------

def serpentine(nrow, ncol):
    """one path through every cell: east along row 0, one step south, west along row 1, ... to the root at the end of the last
    row.  nrow * ncol - 1 steps."""
    d = np.empty((nrow, ncol), dtype=np.int8)
    for r in range(nrow):
        east = r % 2 == 0
        d[r, :] = 0 if east else 4
        d[r, -1 if east else 0] = 2
    d[nrow - 1, -1 if (nrow - 1) % 2 == 0 else 0] = hr.DIR_OUT
    return d


def random_forest(rng, nrow, ncol, p_na=0.1):
    """a well-formed direction plane: every cell gets a distinct random height, NA cells are cut out, a cell points at its
    lowest valid neighbour if that is lower than itself and is a root otherwise"""
    h = rng.permutation(nrow * ncol).reshape(nrow, ncol).astype(np.float64)
    na = rng.random((nrow, ncol)) < p_na
    h[na] = np.inf
    hp = np.full((nrow + 2, ncol + 2), np.inf)
    hp[1:-1, 1:-1] = h
    best = np.full((nrow, ncol), hr.DIR_OUT, dtype=np.int8)
    low = h.copy()
    for k in range(8):
        nb = hp[1 + hr.K_DR[k]:1 + hr.K_DR[k] + nrow, 1 + hr.K_DC[k]:1 + hr.K_DC[k] + ncol]
        better = nb < low
        best[better] = k
        low = np.where(better, nb, low)
    best[na] = hr.DIR_NA
    return best


_HYDRO = {}


def hydro_plane(kind, shape, dx=30.0, dy=30.0):
    """(z, flowdir, flowacc) of a plane of hydro_ref by its restatement, made once per session"""
    key = (kind, tuple(shape), dx, dy)
    if key not in _HYDRO:
        z = hr.spiral(shape[0]) if kind == "spiral" else hr.plane(kind, shape)
        h = hr.hydro(z, np.nan, dx, dy)
        _HYDRO[key] = (z, h["flowdir"], h["flowacc"])
    return _HYDRO[key]
