"""The hydrology rules of include/machisplin_hip.h (section "hydrology") restated by OTHER algorithms than the library's
tile sweeps, so that agreement is a real check: the filled surface by a priority flood with a heap (Barnes, Lehman & Mulla
2014), the flat distance by a breadth-first search from the seeds, the direction rule in numpy, the accumulation by one walk
through the cells in topological order ((W, D) descending).  Every arithmetic operation stands in the header's order and is
rounded once, so the device planes must equal these bit for bit -- but for the TWI, which goes through log.

Also the planes the tests run on: integer-valued heights, so that int16, float32 and float64 hold the same plane."""
import heapq
from collections import deque

import numpy as np

import terrain_ref as tr

K_DR = (0, 1, 1, 1, 0, -1, -1, -1)            # k = 0 .. 7 = E, SE, S, SW, W, NW, N, NE: rows south ...
K_DC = (1, 1, 0, -1, -1, -1, 0, 1)            # ... and columns east of the centre
DIR_OUT, DIR_NA = -1, -2
D_INF = 2**31 - 1
NODATA = -32768.0
# the test planes, shared by the host and the GPU tests: below, at and beyond the kernels' 32 x 64 tile, ragged last tiles
SHAPES = ((1, 1), (1, 70), (70, 1), (2, 2), (33, 65), (97, 130), (200, 300))
KINDS = ("noise", "tilted", "bowl", "constant", "holes", "all_na")
PLANES = [(k, s) for k in KINDS for s in SHAPES] + [("spiral", (96, 96))]


def _shift(p, k):
    """neighbour k of every cell, from the plane padded by one cell"""
    nr, nc = p.shape[0] - 2, p.shape[1] - 2
    return p[1 + K_DR[k]:1 + K_DR[k] + nr, 1 + K_DC[k]:1 + K_DC[k] + nc]


def _pad(a, fill):
    p = np.full((a.shape[0] + 2, a.shape[1] + 2), fill, dtype=a.dtype)
    p[1:-1, 1:-1] = a
    return p


def outlets(z):
    """valid cells on the raster's outer ring or 8-adjacent to an NA cell: one of the eight is not a neighbour"""
    valid = ~np.isnan(z)
    vp = _pad(valid, False)
    lacking = np.zeros(z.shape, dtype=bool)
    for k in range(8):
        lacking |= ~_shift(vp, k)
    return valid & lacking


def fill(z):
    """W by priority flood: the outlets enter the heap at their own height, the lowest cell on the heap floods its
    unvisited neighbours to max(z, its level)"""
    nr, nc = z.shape
    W = np.full(z.shape, np.nan)
    done = np.isnan(z)
    heap = []
    for r, c in zip(*np.nonzero(outlets(z))):
        W[r, c] = z[r, c]
        done[r, c] = True
        heap.append((z[r, c], int(r), int(c)))
    heapq.heapify(heap)
    while heap:
        w, r, c = heapq.heappop(heap)
        for k in range(8):
            rr, cc = r + K_DR[k], c + K_DC[k]
            if 0 <= rr < nr and 0 <= cc < nc and not done[rr, cc]:
                done[rr, cc] = True
                W[rr, cc] = max(z[rr, cc], w)
                heapq.heappush(heap, (W[rr, cc], rr, cc))
    return W


def flat_distance(W, out):
    """D by breadth-first search: seeds (outlets, cells with a strictly lower neighbour) are 0, a step goes to a neighbour
    of equal W.  NA cells get 0 (never looked at)."""
    nr, nc = W.shape
    wp = _pad(W, np.nan)
    seed = out.copy()
    with np.errstate(invalid="ignore"):
        for k in range(8):
            seed |= _shift(wp, k) < W
    D = np.where(seed | np.isnan(W), 0, D_INF).astype(np.int32)
    queue = deque((int(r), int(c)) for r, c in zip(*np.nonzero(seed)))
    while queue:
        r, c = queue.popleft()
        for k in range(8):
            rr, cc = r + K_DR[k], c + K_DC[k]
            if 0 <= rr < nr and 0 <= cc < nc and D[rr, cc] == D_INF and W[rr, cc] == W[r, c]:
                D[rr, cc] = D[r, c] + 1
                queue.append((rr, cc))
    return D


def direction(W, D, dx, dy, dx_row=None):
    """the direction rule, vectorised over the plane: int8"""
    dxr = tr._dx(W, dx, dx_row)
    g = np.sqrt(dxr * dxr + np.float64(dy) * np.float64(dy))
    dist = (dxr, g, np.float64(dy), g, dxr, g, np.float64(dy), g)
    wp, dp = _pad(W, np.nan), _pad(D, 0)
    best = np.full(W.shape, -1, dtype=np.int64)
    s_best = np.zeros(W.shape)
    with np.errstate(invalid="ignore"):
        for k in range(8):
            s = (W - _shift(wp, k)) / dist[k]
            better = s > s_best                              # false for a NaN: no neighbour
            best = np.where(better, k, best)
            s_best = np.where(better, s, s_best)
        none = best < 0
        for k in range(7, -1, -1):                            # descending, so that the lowest k stays
            along = none & (D > 0) & (_shift(wp, k) == W) & (_shift(dp, k) == D - 1)
            best = np.where(along, k, best)
    return np.where(np.isnan(W), DIR_NA, best).astype(np.int8)


def accumulation(W, D, d8):
    """A by one walk in topological order: (W, D) falls strictly along every step, so sorted by (W, D) descending every
    cell comes after all the cells that drain into it.  int64."""
    nr, nc = W.shape
    A = np.where(np.isnan(W), 0, 1).astype(np.int64)
    rows, cols = np.nonzero(~np.isnan(W))
    order = np.lexsort((-D[rows, cols].astype(np.int64), -W[rows, cols]))
    for i in order:
        r, c = int(rows[i]), int(cols[i])
        k = int(d8[r, c])
        if k >= 0:
            rr, cc = r + K_DR[k], c + K_DC[k]
            assert (W[rr, cc], D[rr, cc]) < (W[r, c], D[r, c])
            A[rr, cc] += A[r, c]
    return A


def hydro(plane, nodata, dx, dy, z_factor=1.0, dx_row=None, min_slope_tan=np.tan(np.deg2rad(0.1))):
    """dict: filled, dist, flowdir, flowacc (float64, NaN at NA cells), twi_arg (what the log is taken of), twi, and the
    counts n_valid, n_raised, n_sinks"""
    z = tr.to_double(plane, nodata)
    out = outlets(z)
    W = fill(z)
    D = flat_distance(W, out)
    d8 = direction(W, D, dx, dy, dx_row)
    A = accumulation(W, D, d8)
    acc = np.where(np.isnan(z), np.nan, A.astype(np.float64))
    t = tr.terrain(W, np.nan, dx, dy, z_factor, dx_row)["slope_tan"]
    dxr = tr._dx(z, dx, dx_row)
    with np.errstate(invalid="ignore"):
        arg = (acc * np.sqrt(dxr * np.float64(dy))) / np.where(t > min_slope_tan, t, np.where(np.isnan(t), np.nan, min_slope_tan))
        twi = np.log(arg)
        raised = int((W > z).sum())
    return {"filled": W, "dist": D, "flowdir": d8, "flowacc": acc, "twi_arg": arg, "twi": twi, "outlets": out,
            "n_valid": int((~np.isnan(z)).sum()), "n_raised": raised, "n_sinks": int((d8 == DIR_OUT).sum())}


def check_invariants(z, h):
    """W >= z; following the directions strictly lowers (W, D); the accumulation over the sinks is the number of valid cells"""
    W, D, d8, A = h["filled"], h["dist"], h["flowdir"], h["flowacc"]
    valid = ~np.isnan(z)
    assert np.array_equal(np.isnan(W), ~valid) and (W[valid] >= z[valid]).all()
    assert (W[h["outlets"]] == z[h["outlets"]]).all() and (D[valid] < D_INF).all() and (D[valid] >= 0).all()
    assert ((d8 == DIR_NA) == ~valid).all() and (d8[valid] >= DIR_OUT).all() and (d8[valid] <= 7).all()
    for r, c in zip(*np.nonzero(d8 >= 0)):
        rr, cc = r + K_DR[d8[r, c]], c + K_DC[d8[r, c]]
        assert 0 <= rr < z.shape[0] and 0 <= cc < z.shape[1] and valid[rr, cc]
        assert (W[rr, cc], D[rr, cc]) < (W[r, c], D[r, c]), (r, c)
    assert np.nansum(A[d8 == DIR_OUT]) == valid.sum() == h["n_valid"]
    assert (d8[valid & (D == 0) & ~h["outlets"]] >= 0).all()             # only an outlet can send its water out


# ---- the planes of the tests: float64 arrays of integer values, NaN = NA ----------------------------------------------

def spiral(n=96):
    """a one-cell-wide channel between walls, spiralling from the centre (highest) to the border (lowest): the channel cell
    reached at step i from the outside has height i, the walls 10 000"""
    z = np.full((n, n), 10000.0)
    chan = np.zeros((n, n), dtype=bool)

    def free(r, c):
        return 0 <= r < n and 0 <= c < n and not chan[r, c]

    # walk clockwise from the north-west corner: straight on while the next cell is free and the one behind it is not
    # channel already (that one stays wall), else turn right; stop when neither way is open
    r, c, dr, dc = 0, 0, 0, 1
    path = [(0, 0)]
    chan[0, 0] = True
    while True:
        for _ in range(2):
            r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if free(r1, c1) and not (0 <= r2 < n and 0 <= c2 < n and chan[r2, c2]):
                break
            dr, dc = dc, -dr
        else:
            break
        r, c = r1, c1
        chan[r, c] = True
        path.append((r, c))
    for i, (r, c) in enumerate(path):
        z[r, c] = float(i)
    return z


def plane(kind, shape):
    """the test planes by name"""
    nr, nc = shape
    rng = np.random.default_rng(7 * nr + nc)
    r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
    if kind == "noise":                                   # uniform integer noise 0 .. 49: many pits
        return rng.integers(0, 50, shape).astype(np.float64)
    if kind == "tilted":                                  # tilted plus noise
        return np.floor(3.0 * r + 2.0 * c) + rng.integers(0, 12, shape)
    if kind == "bowl":                                    # a bowl floored to integers: one lake over several tiles
        return np.floor(0.002 * ((r - nr / 2.0) ** 2 + (c - nc / 2.0) ** 2))
    if kind == "constant":
        return np.full(shape, 17.0)
    if kind == "holes":                                   # tilted plus noise with an NA block and a single NA cell
        z = np.floor(3.0 * r + 2.0 * c) + rng.integers(0, 12, shape)
        z[nr // 3:nr // 3 + max(1, nr // 6), nc // 2:nc // 2 + max(1, nc // 5)] = np.nan
        z[(2 * nr) // 3, nc // 4] = np.nan
        return z
    if kind == "all_na":
        return np.full(shape, np.nan)
    raise ValueError(kind)


def as_dtype(z, dtype):
    """the float64 plane (NaN = NA) as the stack holds it: int16 with the nodata -32768, float32 / float64 with NaN"""
    if dtype == "i16":
        return np.where(np.isnan(z), NODATA, z).astype(np.int16)
    return z.astype({"f32": np.float32, "f64": np.float64}[dtype])
