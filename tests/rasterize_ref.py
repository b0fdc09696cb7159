"""The numpy restatement of the rasterize rule (include/machisplin_hip.h, section "rasterize") that the GPU tests compare with
exactly.  It states the two counts of the centre rule by their DEFINITION -- the number of cell centres left of a crossing, the
number of row centres at or above a y, both by a search in the arrays of the centres themselves -- where the library guesses
with floor() and confirms; it knows nothing of boxes, bit planes or batches.  Each line is the header's sequence of float64
operations (numpy does not contract)."""
import numpy as np

INFO = ("n_features", "n_parts", "n_vertices", "n_edges", "n_items", "n_burned", "n_outside")     # what does not depend on the scratch plan
RULES = ("last", "first", "max", "min")


class Grid:
    def __init__(self, g):
        self.g = g
        self.nrow, self.ncol = g.nrow, g.ncol
        self.xc = g.xmin + (np.arange(g.ncol, dtype=np.float64) + 0.5) * g.xres
        self.yr = g.ymax - (np.arange(g.nrow, dtype=np.float64) + 0.5) * g.yres
        self.yr_up = self.yr[::-1].copy()                                      # ascending

    def cstar(self, X):
        """#{c : x_c(c) < X}"""
        return np.searchsorted(self.xc, X, side="left")

    def rabove(self, y):
        """#{r : y_r(r) >= y}"""
        return self.nrow - np.searchsorted(self.yr_up, y, side="left")

    def yedge(self, r):
        return self.g.ymax - np.asarray(r, dtype=np.float64) * self.g.yres

    def col(self, x):
        return np.clip(np.floor((x - self.g.xmin) / self.g.xres), -1, self.ncol).astype(np.int64)

    def row(self, y):
        return np.clip(np.floor((self.g.ymax - y) / self.g.yres), -1, self.nrow).astype(np.int64)


def segments(xy):
    """the segments of one part in canonical orientation: xa, ya, xb, yb, t"""
    x0, y0, x1, y1 = xy[:-1, 0], xy[:-1, 1], xy[1:, 0], xy[1:, 1]
    swap = y1 < y0
    xa, ya, xb, yb = np.where(swap, x1, x0), np.where(swap, y1, y0), np.where(swap, x0, x1), np.where(swap, y0, y1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(yb > ya, (xb - xa) / (yb - ya), 0.0)
    return xa, ya, xb, yb, t


def X_of(xa, ya, xb, yb, t, y):
    v = xa + (y - ya) * t
    v = np.minimum(np.maximum(v, np.minimum(xa, xb)), np.maximum(xa, xb))
    return np.where(y >= yb, xb, v)


def _expand(first, n):
    """items (edge, row) of edges with rows first .. first + n - 1"""
    e = np.repeat(np.arange(first.size), n)
    start = np.cumsum(n) - n
    return e, first[e] + (np.arange(e.size) - start[e])


def crossings(G, xy):
    """the crossings of one ring with the grid's rows: (rows, c*)"""
    xa, ya, xb, yb, t = segments(xy)
    first = G.rabove(yb)
    n = np.where(yb > ya, G.rabove(ya) - first, 0)
    e, r = _expand(first, n)
    X = X_of(xa[e], ya[e], xb[e], yb[e], t[e], G.yr[r])
    return r, G.cstar(X)


def spans(G, xy):
    """the line items of one part: (rows, c_lo, c_hi) of the spans that burn something, and the number of items"""
    xa, ya, xb, yb, t = segments(xy)
    first = np.maximum(G.row(yb), 0)
    last = np.minimum(G.row(ya), G.nrow - 1)
    n = np.maximum(last - first + 1, 0)
    e, r = _expand(first, n)
    xa, ya, xb, yb, t = xa[e], ya[e], xb[e], yb[e], t[e]
    flat = ~(yb > ya)
    ylo, yhi = np.maximum(ya, G.yedge(r + 1)), np.minimum(yb, G.yedge(r))
    x0 = np.where(flat, xa, X_of(xa, ya, xb, yb, t, ylo))
    x1 = np.where(flat, xb, X_of(xa, ya, xb, yb, t, yhi))
    c_lo, c_hi = np.maximum(G.col(np.minimum(x0, x1)), 0), np.minimum(G.col(np.maximum(x0, x1)), G.ncol - 1)
    keep = (flat | (ylo <= yhi)) & (c_lo <= c_hi)
    return r[keep], c_lo[keep], c_hi[keep], int(e.size)


def cover_of(G, parts, kind, touches=False):
    """the cells one feature covers: (first row, a bool block of rows x ncol) or None, and its number of items"""
    cr, cc, lr, l0, l1 = [], [], [], [], []
    n_items = 0
    for xy in parts:
        if kind == "polygon":
            r, c = crossings(G, xy)
            cr.append(r)
            cc.append(c)
            n_items += r.size
        if kind == "line" or touches:
            r, a, b, n = spans(G, xy)
            lr.append(r)
            l0.append(a)
            l1.append(b)
            n_items += n
    rows = np.concatenate(cr + lr) if cr or lr else np.zeros(0, dtype=np.int64)
    if rows.size == 0:
        return None, n_items
    top, h = int(rows.min()), int(rows.max() - rows.min()) + 1
    cover = np.zeros((h, G.ncol), dtype=bool)
    if cr:
        toggles = np.zeros((h, G.ncol + 1), dtype=np.int64)
        np.add.at(toggles, (np.concatenate(cr) - top, np.concatenate(cc)), 1)
        right = np.cumsum(toggles[:, ::-1], axis=1)[:, ::-1]                   # the toggles at c* >= j
        cover |= (right[:, 1:] & 1).astype(bool)                               # cell c is toggled by every crossing with c < c*
    if lr:
        diff = np.zeros((h, G.ncol + 1), dtype=np.int64)
        np.add.at(diff, (np.concatenate(lr) - top, np.concatenate(l0)), 1)
        np.add.at(diff, (np.concatenate(lr) - top, np.concatenate(l1) + 1), -1)
        cover |= np.cumsum(diff, axis=1)[:, :-1] > 0
    return (top, cover), n_items


def keys_of(n, rule, values):
    i = np.arange(n, dtype=np.int64)
    if rule == "last":
        return i
    if rule == "first":
        return n - 1 - i
    order = np.lexsort((i, np.asarray(values, dtype=np.float64)))              # by value, ties by index
    rank = np.empty(n, dtype=np.int64)
    rank[order] = i
    return rank if rule == "max" else n - 1 - rank


def point_cells(g, xy):
    """(row, col, inside) by terra's colFromX / rowFromY"""
    x, y = xy[:, 0], xy[:, 1]
    xmax, ymin = g.xmin + g.ncol * g.xres, g.ymax - g.nrow * g.yres
    inside = ~((x < g.xmin) | (x > xmax) | (y < ymin) | (y > g.ymax))
    c = np.where(x == xmax, g.ncol - 1, np.clip(np.floor((x - g.xmin) / g.xres), -1, g.ncol)).astype(np.int64)
    r = np.where(y == ymin, g.nrow - 1, np.clip(np.floor((g.ymax - y) / g.yres), -1, g.nrow)).astype(np.int64)
    inside &= (c >= 0) & (c < g.ncol) & (r >= 0) & (r < g.nrow)
    return r, c, inside


def feature_parts(ft, i):
    return [ft.coords[ft.part_offsets[p]:ft.part_offsets[p + 1]] for p in range(ft.feature_offsets[i], ft.feature_offsets[i + 1])]


def rasterize(ft, g, rule="last", touches=False, out_dtype=np.float64):
    """every product and the info: ({"index", "count", "value"}, info).  ``value`` only when the features carry values."""
    G = Grid(g)
    n = ft.n_features
    keys = keys_of(n, rule, ft.values)
    key = np.full((g.nrow, g.ncol), -1, dtype=np.int64)
    count = np.zeros((g.nrow, g.ncol), dtype=np.int32)
    n_items = n_outside = 0
    if ft.kind == "point":
        feat = np.repeat(np.arange(n), np.diff(ft.part_offsets[ft.feature_offsets]))
        r, c, inside = point_cells(g, ft.coords)
        np.maximum.at(key, (r[inside], c[inside]), keys[feat[inside]])
        np.add.at(count, (r[inside], c[inside]), 1)
        n_items, n_outside = ft.n_vertices, int((~inside).sum())
    else:
        for i in range(n):
            got, k = cover_of(G, feature_parts(ft, i), ft.kind, touches and ft.kind == "polygon")
            n_items += k
            if got is None:
                continue
            top, cover = got
            block = key[top:top + cover.shape[0]]
            block[cover] = np.maximum(block[cover], keys[i])
            count[top:top + cover.shape[0]] += cover
    feature_of = np.empty(max(n, 1), dtype=np.int64)
    feature_of[keys] = np.arange(n)
    index = np.where(key >= 0, feature_of[np.maximum(key, 0)], -1).astype(np.int32)
    planes = {"index": index, "count": count}
    if ft.values is not None:
        planes["value"] = np.where(index >= 0, ft.values[np.maximum(index, 0)] if n else np.nan, np.nan).astype(out_dtype)
    info = {"n_features": n, "n_parts": ft.n_parts, "n_vertices": ft.n_vertices, "n_edges": 0 if ft.kind == "point" else ft.n_vertices - ft.n_parts,
            "n_items": int(n_items), "n_burned": int((key >= 0).sum()), "n_outside": n_outside}
    return planes, info


# ---- shapes the tests share ------------------------------------------------------------------------------------------------

def star(cx, cy, r_in, r_out, n, seed=0, close=True):
    """a star-shaped ring of n vertices (+ the closing one) around (cx, cy), radii jittered between r_in and r_out"""
    rng = np.random.default_rng(seed)
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    rad = rng.uniform(r_in, r_out, n)
    xy = np.column_stack([cx + rad * np.cos(a), cy + rad * np.sin(a)])
    return np.vstack([xy, xy[:1]]) if close else xy


def lattice(g, ny, nx, seed=0, jitter=0.25, zigzag=0):
    """a partition of the grid's extent into ny x nx polygons whose neighbours share their edges vertex by vertex: the nodes of
    a regular lattice, the inner ones jittered, each edge with `zigzag` extra jittered vertices; neighbours walk a shared edge in
    opposite directions.  Returns the list of rings (one per polygon, row-major)."""
    rng = np.random.default_rng(seed)
    xmax, ymin = g.xmin + g.ncol * g.xres, g.ymax - g.nrow * g.yres
    sx, sy = (xmax - g.xmin) / nx, (g.ymax - ymin) / ny
    X = g.xmin + np.arange(nx + 1) * sx + np.zeros((ny + 1, 1))
    Y = g.ymax - np.arange(ny + 1)[:, None] * sy + np.zeros((1, nx + 1))
    X[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (ny - 1, nx - 1)) * sx
    Y[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (ny - 1, nx - 1)) * sy
    X[:, 0], X[:, -1], Y[0, :], Y[-1, :] = g.xmin, xmax, g.ymax, ymin

    def edge(p, q, inner):
        """vertices from p to q (q excluded), the same whichever polygon asks"""
        if not zigzag:
            return [p]
        lo, hi = (p, q) if p <= q else (q, p)
        r = np.random.default_rng([seed, lo[0], lo[1], hi[0], hi[1]])
        f = np.sort(r.uniform(0.1, 0.9, zigzag))
        a, b = np.array([X[lo], Y[lo]]), np.array([X[hi], Y[hi]])
        pts = a + f[:, None] * (b - a)
        if inner:
            pts = pts + r.uniform(-0.08, 0.08, (zigzag, 2)) * np.array([sx, sy])
        pts = [tuple(v) for v in pts]
        return [p] + (pts if p == lo else pts[::-1])

    rings = []
    for i in range(ny):
        for j in range(nx):
            nodes = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)]
            ring = []
            for a, b in zip(nodes, nodes[1:] + nodes[:1]):
                inner = not ((a[0] == b[0] and a[0] in (0, ny)) or (a[1] == b[1] and a[1] in (0, nx)))
                for v in edge(a, b, inner):
                    ring.append((X[v], Y[v]) if isinstance(v[0], (int, np.integer)) else v)
            ring.append(ring[0])
            rings.append(np.array(ring, dtype=np.float64))
    return rings
