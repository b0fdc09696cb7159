"""Host restatements of the three hand-made approximations under the spline and ksvm kernels (test infrastructure
only: the product never imports it).

  * the table log: build_log_table (csrc/runtime.hip), table_log_biased / r2logr2 (csrc/devmath.h);
  * the table exp: the 4096-entry table of runtime.hip, table_exp_neg_acc and the exponent argument of svr_kernel
    (csrc/ensemble.hip) with mhs_svr_load's per-vector record (csrc/models.hip);
  * the far-field rule of csrc/tps_eval.hip: far_plan_choose, far_plan_sort, cheb_matrix, the nodes of ff_nodes_block
    and the  Ly F Lx'  sum of ff_cells_block -- once in float64 in the kernel's order, once in long double.

Every device operation is restated as one correctly rounded float64 operation.  Python's float +, -, *, / are that
already (the library is built without contraction); an fma is the exact product and sum in fractions.Fraction, rounded
once by float().  numpy and the standard library only."""
import math
import struct
from fractions import Fraction

import numpy as np

LD = np.longdouble


def fma(a, b, c):
    """a * b + c rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def ulp(x):
    """spacing of the doubles at |x|"""
    x = abs(float(x))
    return math.ulp(x)


# ------------------------------------------------------------------------------------------------ table log --
LOG_TAB_BITS = 10
LOG_TAB_N = 1 << LOG_TAB_BITS
LN2_D = 0.6931471805599453094
LOG_BIAS_D = -1023.0 * LN2_D
THIRD = 1.0 / 3.0

_log_table = None


def log_table():
    """build_log_table: per bin i the pair (2^1023 * invc, logc) with c the bin's midpoint in long double,
    invc = (double)(1 / c) and logc = (double)(-logl(invc))."""
    global _log_table
    if _log_table is None:
        i = np.arange(LOG_TAB_N, dtype=LD)
        c = LD(1.0) + (i + LD(0.5)) / LD(LOG_TAB_N)
        invc = (LD(1.0) / c).astype(np.float64)
        logc = (-np.log(invc.astype(LD))).astype(np.float64)
        _log_table = (np.ldexp(invc, 1023), logc)
    return _log_table


def log_bin(d2):
    """(biased exponent, bin) that table_log_biased reads off the high word of d2 >= 0"""
    hi = _bits(d2) >> 32
    return hi >> 20, (hi >> (20 - LOG_TAB_BITS)) & (LOG_TAB_N - 1)


def table_log_biased(d2, parts=False):
    """log(d2) + 1023 ln 2 as the device forms it"""
    tx, ty = log_table()
    hi = _bits(d2) >> 32
    e, i = log_bin(d2)
    # invc: the argument's exponent field subtracted from the high word of 2^1023 / c_i
    invc = _from_bits(_bits(float(tx[i])) - ((hi & 0x7FF00000) << 32))
    r = fma(d2, invc, -1.0)
    q = fma(r, THIRD, -0.5)
    r2 = r * r
    lp = fma(r2, q, r)
    L = fma(float(e), LN2_D, float(ty[i]))
    out = L + lp
    return (out, r, lp, L) if parts else out


def r2logr2(d2):
    """d2 log d2, 0 at d2 == 0"""
    return d2 * (table_log_biased(d2) + LOG_BIAS_D)


TPS_KK = 0.5 / (8.0 * math.pi)      # upload_knots: cw = c * (0.5 / (8 pi))


def tps_one_knot_point(x, c=1.0):
    """tps_eval_points_kernel for the one-knot spline of the tests (knot (0, 0), d = 0, centre 0, scale 1) at (x, 0)"""
    cw = c * TPS_KK
    u = (x - 0.0) / 1.0
    dx = u - 0.0
    dd = fma(0.0, 0.0, dx * dx)
    acc = fma(cw, r2logr2(dd), 0.0)
    return 0.0 + 0.0 * u + 0.0 * 0.0 + acc


def log_sweep_points():
    """The x of the log tests (d2 = fl(x * x)): per bin of the table at exponent 0 the smallest d2 at or above the bin's
    lower edge, the largest below its upper edge and one near its middle; eight mantissas at every binary exponent
    -1022 .. 1000 of d2 (1, just under 2, and six drawn at random).  About 19 000 points, always the same."""
    xs = []
    for i in range(LOG_TAB_N):
        lo, up = 1.0 + i / LOG_TAB_N, 1.0 + (i + 1) / LOG_TAB_N
        x = math.sqrt(lo)
        while x * x >= lo:
            x = math.nextafter(x, 0.0)
        while x * x < lo:
            x = math.nextafter(x, 2.0)
        xs.append(x)
        x = math.sqrt(up)
        while x * x < up:
            x = math.nextafter(x, 2.0)
        while x * x >= up:
            x = math.nextafter(x, 0.0)
        xs.append(x)
        xs.append(math.sqrt(0.5 * (lo + up)))
    rng = np.random.default_rng(20240)
    for E in range(-1022, 1001):
        ms = [1.0, math.nextafter(2.0, 0.0)] + list(1.0 + rng.random(6))
        for m in ms:
            h = E // 2
            x = math.ldexp(math.sqrt(m * (2.0 if E & 1 else 1.0)), h)
            d2 = x * x
            # sqrt rounds: step x until fl(x * x) has the exponent asked for (where a double x with that square exists)
            for _ in range(4):
                ex = math.frexp(d2)[1] - 1
                if ex == E or d2 == 0.0:
                    break
                x = math.nextafter(x, math.inf if ex < E else 0.0)
                d2 = x * x
            xs.append(x)
    return np.array(xs)


# ------------------------------------------------------------------------------------------------ table exp --
EXP_TAB_BITS = 12
EXP_TAB_N = 1 << EXP_TAB_BITS
EXP_RANGE = 700.0
EXP_SCALE = 4096.0 / LN2_D
EXP_MAGIC = float(0x3 << 51) + 1023.0 * EXP_TAB_N
EXP_NK = -EXP_RANGE * EXP_SCALE
EXP_C1 = 1.0 / EXP_SCALE
EXP_C2 = 0.5 / (EXP_SCALE * EXP_SCALE)

_exp_table = None


def exp_table():
    """2^(j / 4096) as runtime.hip stores it: (double)exp2l(j / 4096)"""
    global _exp_table
    if _exp_table is None:
        j = np.arange(EXP_TAB_N, dtype=LD)
        _exp_table = np.exp2(j / LD(4096.0)).astype(np.float64)
    return _exp_table


def table_exp_neg_acc(u, acc=0.0, parts=False):
    """acc + exp(-700 u), u in [0, 1], as the device forms it"""
    tab = exp_table()
    t = fma(u, EXP_NK, EXP_MAGIC)                   # the 1.5 * 2^52 rounding: k lands in t's low word
    kd = t - EXP_MAGIC
    k8 = ((_bits(t) & 0xFFFFFFFF) << 8) & 0xFFFFFFFF
    r = fma(u, EXP_NK, -kd)
    j = (k8 >> 8) & (EXP_TAB_N - 1)                 # ubfe(k8, 5, 15) is the byte offset 8 j
    mj = _bits(float(tab[j])) & 0x000FFFFFFFFFFFFF  # the table holds the mantissa bits only
    sj = _from_bits(((k8 & 0xFFF00000) << 32) | mj)
    q = fma(r, EXP_C2, EXP_C1)
    q = fma(q, r, 1.0)
    out = fma(sj, q, acc)
    if parts:
        k = int(kd)
        return out, k >> EXP_TAB_BITS, j, r
    return out


def svr_record(alpha, sv, sigma):
    """mhs_svr_load: the kept support vectors (alpha > 0 first, then alpha < 0), per vector [b_0 .. b_{p-1}, a], and
    (records, npos, amax)"""
    alpha = [float(a) for a in alpha]
    sv = np.asarray(sv, dtype=np.float64)
    amax = max(abs(a) for a in alpha)
    order = [v for v, a in enumerate(alpha) if a > 0]
    npos = len(order)
    order += [v for v, a in enumerate(alpha) if a < 0]
    rec = []
    for v in order:
        ss, b = 0.0, []
        for x in sv[v]:
            x = float(x)
            b.append(-2.0 * sigma * x / EXP_RANGE)
            ss += x * x
        rec.append(b + [(sigma * ss - math.log(abs(alpha[v]) / amax)) / EXP_RANGE])
    return rec, npos, amax


def svr_argument(sp, x, q):
    """the clamped exponent argument of svr_kernel for one record sp and scaled predictors x: the LAT term first"""
    P = len(x)
    arg = q + fma(sp[P - 1], x[P - 1], sp[P])
    for j in range(P - 1):
        arg = fma(sp[j], x[j], arg)
    return min(max(arg, 0.0), 1.0)


def svr_predict(alpha, sv, b, sigma, x_center, x_scale, y_center, y_scale, X):
    """svr_kernel at the rows of X, operation for operation"""
    rec, npos, amax = svr_record(alpha, sv, sigma)
    P = len(x_center)
    sq = sigma / EXP_RANGE
    out = np.empty(len(X))
    for n, row in enumerate(np.asarray(X, dtype=np.float64)):
        x, q = [], 0.0
        for j in range(P):
            x.append((float(row[j]) - float(x_center[j])) / float(x_scale[j]))
            q = fma(x[j], x[j], q)
        q = sq * q
        acc = accn = 0.0
        for v, sp in enumerate(rec):
            if v < npos:
                acc = table_exp_neg_acc(svr_argument(sp, x, q), acc)
            else:
                accn = table_exp_neg_acc(svr_argument(sp, x, q), accn)
        out[n] = ((acc - accn) * amax - b) * y_scale + y_center
    return out


def exp_targets():
    """(e, j, r) of the exp sweep: every table entry j with r near -0.5, 0 and +0.5, the exponent e cycling through
    0 .. -1010 (where -700 * 4096 / ln 2 allows the pair), then every e once more"""
    ymin = EXP_NK + 1.0
    out = []
    for j in range(EXP_TAB_N):
        for n, r in enumerate((-0.5 + 1e-6, 0.0, 0.5 - 1e-6)):
            e = -((3 * j + n) % 1011)
            while 4096 * e + j + r > 0.0:
                e -= 1
            while 4096 * e + j + r < ymin:
                e += 1
            out.append((e, j, r))
    for e in range(0, -1011, -1):
        j = 0 if e == 0 else 200
        out.append((e, j, -0.25))
    return out


def exp_sweep_points():
    """The t of the exp tests (u = fl(t * t); the tests' models have sigma = 700, so q = u): exp_targets, then u = 0,
    the largest t with u <= 1, u = 1 and three arguments beyond 1."""
    ts = [math.sqrt((4096 * e + j + r) / EXP_NK) for e, j, r in exp_targets()]
    ts += [0.0, math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 1.25, 1e10]
    return np.array(ts)


# ------------------------------------------------------------------------------------------- far-field rule --
FF_N = 16
FF_NODES = FF_N * FF_N
FF_PAD = 2


class Geom:
    """EvalGeom of a whole-grid window"""

    def __init__(self, xmin, ymax, xres, yres, nr, nc, center=(0.0, 0.0), scale=(1.0, 1.0), r0=0, c0=0):
        self.xmin, self.ymax, self.xres, self.yres = float(xmin), float(ymax), float(xres), float(yres)
        self.nr, self.nc, self.r0, self.c0 = int(nr), int(nc), int(r0), int(c0)
        self.cx, self.cy, self.sx, self.sy = float(center[0]), float(center[1]), float(scale[0]), float(scale[1])


def cheb_points():
    """FarGeom.t: cos((2 a + 1) pi / 32)"""
    return [math.cos((2 * a + 1) * math.pi / (2.0 * FF_N)) for a in range(FF_N)]


def _llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def far_plan_choose(knots_uv, e, forced=True, lo=0.8, hi=1.25):
    """far_plan_choose with mhs_tps_eval_mode(2) (forced) or 0: None where the direct sum runs, else a dict with the
    tile shape (tx, ty), the tile counts and the knots in window cell coordinates (kc, kr)"""
    kn = np.asarray(knots_uv, dtype=np.float64)
    N = len(kn)
    if e.nc < 64 or e.nr < 16 or N < 32:
        return None
    kc = (kn[:, 0] * e.sx + e.cx - e.xmin) / e.xres - float(e.c0)
    kr = (e.ymax - (kn[:, 1] * e.sy + e.cy)) / e.yres - float(e.r0)
    inside = int(np.count_nonzero((kc >= 0) & (kc < e.nc) & (kr >= 0) & (kr < e.nr)))
    cells = float(e.nr) * float(e.nc)
    rho = float(inside if inside > 0 else 1) / cells
    aspect = (e.xres / e.sx) / (e.yres / e.sy)
    best, btx, bty = 1e300, 0, 0
    for tx in range(64, 1025, 64):
        ty = _llround(float(tx) * aspect / 16.0) * 16
        if ty < 16:
            ty = 16
        if ty > 4096:
            continue
        ntx, nty = math.ceil(e.nc / tx), math.ceil(e.nr / ty)
        cost = ntx * nty * FF_NODES * float(N) / cells + 9.0 * rho * tx * ty + 4.0
        if cost < best:
            best, btx, bty = cost, tx, ty
    if btx == 0:
        return None
    if not forced and best > 0.5 * N:
        return None
    tile_aspect = (float(btx) * e.xres / e.sx) / (float(bty) * e.yres / e.sy)
    if tile_aspect > hi or tile_aspect < lo:
        return None
    return {"tx": btx, "ty": bty, "ntx": (e.nc + btx - 1) // btx, "nty": (e.nr + bty - 1) // bty, "kc": kc, "kr": kr,
            "tile_aspect": tile_aspect}


def far_plan_sort(plan):
    """far_plan_sort: (bin of every knot, start offsets per bin, order) -- bins beyond FF_PAD tiles outside the window
    collapse onto the rim; order[p] = index of the knot at sorted position p (a stable counting sort)"""
    nbx, nby = plan["ntx"] + 2 * FF_PAD, plan["nty"] + 2 * FF_PAD
    bx = np.clip(np.floor(plan["kc"] / plan["tx"]), -FF_PAD, plan["ntx"] + FF_PAD - 1).astype(int)
    by = np.clip(np.floor(plan["kr"] / plan["ty"]), -FF_PAD, plan["nty"] + FF_PAD - 1).astype(int)
    b = (by + FF_PAD) * nbx + (bx + FF_PAD)
    start = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=nbx * nby))])
    return b, start, np.argsort(b, kind="stable")


def tile_far_near(plan, start, txi, tyi):
    """sorted positions of the far knots of tile (txi, tyi), in the order ff_nodes_block sums them, and of its near
    knots (the 3 x 3 block), in ff_cells_block's order"""
    nbx = plan["ntx"] + 2 * FF_PAD
    far, near, j = [], [], 0
    for r in range(3):
        b = (tyi + FF_PAD - 1 + r) * nbx + (txi + FF_PAD - 1)
        far += range(j, start[b])
        near += range(start[b], start[b + 3])
        j = start[b + 3]
    far += range(j, start[-1])
    return far, near


def cheb_matrix(cells, flip, t, dtype=np.float64):
    """cheb_matrix: L[i][a] = l_a(tau_i), barycentric, tau_i the centre of cell i of `cells` mapped to (-1, 1)"""
    if dtype is LD:
        pi = LD(np.pi) + LD(1.2246467991473532e-16)          # pi to long double
        w = [LD(-1.0 if a & 1 else 1.0) * np.sin(LD(2 * a + 1) * pi / LD(2 * FF_N)) for a in range(FF_N)]
    else:
        w = [(-1.0 if a & 1 else 1.0) * math.sin((2 * a + 1) * math.pi / (2.0 * FF_N)) for a in range(FF_N)]
    L = np.zeros((cells, FF_N), dtype=dtype)
    for i in range(cells):
        tau = dtype(2.0 * i + 1.0) / dtype(cells) - dtype(1.0)
        if flip:
            tau = -tau
        q, s, hit = [], dtype(0.0), -1
        for a in range(FF_N):
            d = tau - t[a]
            if d == 0.0:
                hit = a
                break
            q.append(w[a] / d)
            s = s + q[a]
        for a in range(FF_N):
            L[i, a] = (1.0 if a == hit else 0.0) if hit >= 0 else q[a] / s
    return L


def ff_node_coords(e, plan, txi, tyi, t):
    """scaled coordinates (u[a], v[b]) of a tile's nodes as ff_nodes_block forms them"""
    tx, ty = plan["tx"], plan["ty"]
    hx, hy = 0.5 * float(tx) * e.xres, 0.5 * float(ty) * e.yres
    xc = e.xmin + float(e.c0 + txi * tx) * e.xres + hx
    yc = e.ymax - float(e.r0 + tyi * ty) * e.yres - hy
    u = [(xc + hx * t[a] - e.cx) / e.sx for a in range(FF_N)]
    v = [(yc + hy * t[b] - e.cy) / e.sy for b in range(FF_N)]
    return u, v


def cell_coords(e, cols, rows):
    """scaled coordinates of cell centres as every grid kernel forms them"""
    u = [((e.xmin + (float(e.c0 + c) + 0.5) * e.xres) - e.cx) / e.sx for c in cols]
    v = [((e.ymax - (float(e.r0 + r) + 0.5) * e.yres) - e.cy) / e.sy for r in rows]
    return u, v


def tps_accumulate(knots, idx, u, v, acc):
    """tps_accumulate for one cell: acc += sum_j cw_j phi(|(u, v) - knot_j|^2), knots = rows (u, v, cw)"""
    for j in idx:
        ku, kv, cw = knots[j]
        dx = u - ku
        dy = v - kv
        dd = fma(dy, dy, dx * dx)
        acc = fma(cw, r2logr2(dd), acc)
    return acc


def far_tile_f64(e, plan, knots_uv, c, d3, txi, tyi, rows=None):
    """The far-field path's values on tile (txi, tyi) in float64, in the kernels' order: the far knots (and the affine
    part) summed at the 256 nodes, G = F Lx', Ly G, then the near knots added directly.  rows: tile rows to evaluate
    (default all).  Returns (values, Lx, Ly, F)."""
    b, start, order = far_plan_sort(plan)
    kn = np.asarray(knots_uv, dtype=np.float64)[order]
    knots = [(float(p[0]), float(p[1]), float(cj) * TPS_KK) for p, cj in zip(kn, np.asarray(c, dtype=np.float64)[order])]
    far, near = tile_far_near(plan, start, txi, tyi)
    t = cheb_points()
    un, vn = ff_node_coords(e, plan, txi, tyi, t)
    F = np.empty((FF_N, FF_N))
    for bb in range(FF_N):
        for a in range(FF_N):
            F[bb, a] = d3[0] + d3[1] * un[a] + d3[2] * vn[bb] + tps_accumulate(knots, far, un[a], vn[bb], 0.0)
    tx, ty = plan["tx"], plan["ty"]
    Lx, Ly = cheb_matrix(tx, False, t), cheb_matrix(ty, True, t)
    rows = range(ty) if rows is None else rows
    uc, vc = cell_coords(e, range(txi * tx, (txi + 1) * tx), [tyi * ty + r for r in rows])
    G = np.empty((FF_N, tx))
    for bb in range(FF_N):
        for i in range(tx):
            s = 0.0
            for a in range(FF_N):
                s = fma(float(F[bb, a]), float(Lx[i, a]), s)
            G[bb, i] = s
    out = np.empty((len(rows), tx))
    for k, r in enumerate(rows):
        for i in range(tx):
            s = 0.0
            for bb in range(FF_N):
                s = fma(float(Ly[r, bb]), float(G[bb, i]), s)
            out[k, i] = tps_accumulate(knots, near, uc[i], vc[k], s)
    return out, Lx, Ly, F


def phi_sum_ld(knots_uv, c, u, v, absolute=False):
    """sum_j c_j (1 / 16 pi) r^2 log r^2 at the points u[None, :] x v[:, None] in long double (float64 coordinates,
    as the device has them); absolute: sum_j |c_j phi_j|"""
    u, v = np.asarray(u, dtype=LD)[None, :], np.asarray(v, dtype=LD)[:, None]
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    kk = LD(0.5) / (LD(8.0) * pi)
    s = np.zeros((v.shape[0], u.shape[1]), dtype=LD)
    for (ku, kv), cj in zip(np.asarray(knots_uv, dtype=np.float64), np.asarray(c, dtype=np.float64)):
        d2 = (u - LD(ku)) ** 2 + (v - LD(kv)) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            ph = np.where(d2 > 0, d2 * np.log(d2), LD(0.0)) * kk * LD(cj)
        s = s + (np.abs(ph) if absolute else ph)
    return s


def far_method_error(e, plan, knots_uv, c, txi, tyi):
    """The interpolant's own error on tile (txi, tyi): the long-double 16 x 16 Chebyshev interpolant of the far knots'
    sum (long-double nodes and weights) against that sum itself, as a share of sum_j |c_j phi_j| over the tile's far
    knots (the largest over the tile's cells of each).  Returns (share, far knot indices, near knot indices)."""
    b, start, order = far_plan_sort(plan)
    far, near = tile_far_near(plan, start, txi, tyi)
    fi, ni = order[far], order[near]
    kn, c = np.asarray(knots_uv, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return _interp_error_ld(e, plan, kn[fi], c[fi], txi, tyi), fi, ni


def far_single_knot_error(e, plan, knots_uv, txi, tyi):
    """far_method_error for each far knot of the tile alone: the largest share of that knot's max |phi| on the tile"""
    b, start, order = far_plan_sort(plan)
    far, near = tile_far_near(plan, start, txi, tyi)
    kn = np.asarray(knots_uv, dtype=np.float64)
    return max(_interp_error_ld(e, plan, kn[j:j + 1], np.ones(1), txi, tyi) for j in order[far])


def _interp_error_ld(e, plan, kn, c, txi, tyi):
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    t = [np.cos(LD(2 * a + 1) * pi / LD(2 * FF_N)) for a in range(FF_N)]
    tx, ty = plan["tx"], plan["ty"]
    hx, hy = LD(0.5) * LD(tx) * LD(e.xres), LD(0.5) * LD(ty) * LD(e.yres)
    xc = LD(e.xmin) + LD(e.c0 + txi * tx) * LD(e.xres) + hx
    yc = LD(e.ymax) - LD(e.r0 + tyi * ty) * LD(e.yres) - hy
    un = np.array([(xc + hx * ta - LD(e.cx)) / LD(e.sx) for ta in t], dtype=LD)
    vn = np.array([(yc + hy * ta - LD(e.cy)) / LD(e.sy) for ta in t], dtype=LD)
    F = _phi_sum_ld_exact(kn, c, un, vn)
    Lx, Ly = _cheb_ld(tx, False), _cheb_ld(ty, True)
    interp = Ly @ F @ Lx.T
    uc, vc = cell_coords(e, range(txi * tx, (txi + 1) * tx), range(tyi * ty, (tyi + 1) * ty))
    exact = phi_sum_ld(kn, c, uc, vc)
    S = phi_sum_ld(kn, c, uc, vc, absolute=True)
    return float(np.abs(interp - exact).max() / S.max())


_cheb_cache = {}


def _cheb_ld(cells, flip):
    if (cells, flip) not in _cheb_cache:
        pi = LD(np.pi) + LD(1.2246467991473532e-16)
        t = [np.cos(LD(2 * a + 1) * pi / LD(2 * FF_N)) for a in range(FF_N)]
        _cheb_cache[(cells, flip)] = cheb_matrix(cells, flip, t, LD)
    return _cheb_cache[(cells, flip)]


def _phi_sum_ld_exact(kn, c, u, v):
    """phi_sum_ld at long-double coordinates"""
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    kk = LD(0.5) / (LD(8.0) * pi)
    s = np.zeros((len(v), len(u)), dtype=LD)
    for (ku, kv), cj in zip(kn, c):
        d2 = (u[None, :] - LD(ku)) ** 2 + (v[:, None] - LD(kv)) ** 2
        s = s + d2 * np.log(d2) * kk * LD(cj)
    return s


FAR_K4 = (4.0, 2.49, 2.51)          # 4 * aspect of the three layouts: tiles of 64 x 64, 64 x 32 and 64 x 48 cells


def far_layout(k4):
    """The worst accepted geometry of the far-field rule: 5 x 5 tiles of 64 columns by ty rows, centre 0, scale 1,
    yres = 2^-6 and xres = k4 * 2^-8, so 4 * aspect = k4.  Knots (all c > 0): along the four edges of the ring of bins at
    Chebyshev distance 2 from the centre tile that face it, within one cell of the edge -- among them points 2^-30 of a cell
    inside the left and upper edge and points exactly on the right and lower edge (cell coordinate 256 and
    4 ty: the first of a far bin) --, four exactly on the edges of the 3 x 3 block's own bins (cell coordinate 64 and ty:
    near knots of the centre tile), and four more than two tiles outside the window (rim bins).
    Returns (Geom, ty, knots n x 2, c)."""
    yres, xres = 2.0 ** -6, k4 * 2.0 ** -8
    ty = _llround(k4) * 16
    nr, nc = 5 * ty, 320
    e = Geom(0.0, nr * yres, xres, yres, nr, nc)
    pts = []                                             # (column, row) in cell coordinates
    below = lambda x: x - 2.0 ** -30                     # (the nearest double below may come back as x from the plan's division)
    fr = [0.0, 0.125, 0.3, 0.5, 0.7, 0.875, 1.0 - 2.0 ** -30]
    for f in fr:                                         # alongside the centre tile and the tiles next to it
        r = (2.0 + f) * ty
        pts += [(below(64.0), r), (256.0, r)]
        cc = (2.0 + f) * 64.0
        pts += [(cc, below(float(ty))), (cc, 4.0 * ty)]
    for f in (0.25, 0.75):
        pts += [(63.5, (1.0 + f) * ty), (256.5, (3.0 + f) * ty), ((1.0 + f) * 64.0, ty - 0.5), ((3.0 + f) * 64.0, 4.0 * ty + 0.5)]
    pts += [(63.25, ty - 0.75), (256.75, ty - 0.25), (63.75, 4.0 * ty + 0.25), (256.25, 4.0 * ty + 0.75)]     # the ring's corners
    pts += [(64.0, 2.5 * ty), (160.0, float(ty)), (64.0, float(ty)), (100.0, 2.0 * ty)]                      # on bin edges, near
    pts += [(-150.0, 2.5 * ty), (320.0 + 135.0, 0.5 * ty), (160.0, -2.2 * ty), (30.0, 7.3 * ty)]              # rim bins
    pts = np.array(pts)
    kn = np.column_stack([e.xmin + pts[:, 0] * xres, e.ymax - pts[:, 1] * yres])
    c = 0.5 + np.random.default_rng(7).random(len(kn))
    return e, ty, kn, c
