"""The table log, the table exp and the far-field rule, restated on the host (tests/devmath_ref.py), against a
high-precision reference and against bounds derived from the arithmetic.  CPU only.

Every bound below is  truncation of the polynomial + a counted number of half-ulps, each at the magnitude where the
rounding happens;  none is read off the code under test.  The measured maxima must lie under the bound and above a
tenth of it, and are written to profiles/devmath_bounds.txt."""
import functools
import math
import os

import numpy as np
import pytest

import devmath_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(os.path.dirname(HERE), "profiles", "devmath_bounds.txt")

try:
    import mpmath as mp
    mp.mp.dps = 50
    REF = "mpmath, 50 digits"
except ImportError:
    mp = None
    REF = "numpy long double"


def _log_err(val, d2):
    """val - log(d2)"""
    if mp is not None:
        return float(mp.mpf(val) - mp.log(mp.mpf(d2)))
    return float(R.LD(val) - np.log(R.LD(d2)))


def _exp_relerr(val, u):
    """val / exp(-700 u) - 1"""
    if mp is not None:
        return float(mp.mpf(val) / mp.exp(-700 * mp.mpf(u)) - 1)
    return float(R.LD(val) / np.exp(R.LD(-700.0) * R.LD(u)) - R.LD(1.0))


def _hu(x):
    """half an ulp at the magnitude of x (of the next binade where x is within 1e-6 of it: x is itself approximate)"""
    return 0.5 * np.spacing(np.abs(x) * (1.0 + 1e-6))


def log_bound(d2):
    """Bound on |table_log_biased(d2) + LOG_BIAS_D - log d2| for a normal d2 with biased exponent e, from devmath.h:

      truncation   log1p(r) - (r - r^2/2 + r^3/3), |r| <= 2^-11 (half a bin over c >= 1):  r^4 / 4 / (1 - |r|) <= 2^-46 (1 + 2^-9)
      logc         the table entry: half an ulp below 1 (2^-54), logl's own error and the second rounding below 2^-63
      r, q, r2, lp four roundings that reach the result at no more than half an ulp of 2^-11 each: 4 * 2^-65
      L            fma(e, LN2_D, logc): half an ulp at e ln 2 + logc (1.1e-13 * 0.5 at 709)
      L + lp       half an ulp at the same magnitude
      LN2_D        the literal is within half an ulp (2^-54) of ln 2, and enters e times in L and 1023 times, negated,
                   in LOG_BIAS_D: |e - 1023| * 2^-54
      LOG_BIAS_D   fl(-1023 LN2_D): half an ulp at 709
      + LOG_BIAS_D half an ulp at |log d2|"""
    e = np.frexp(d2)[1] - 1 + 1023                   # (d2 a double or an array of them)
    L = e * math.log(2.0) + 0.7
    trunc = 2.0 ** -46 * (1.0 + 2.0 ** -9)
    return (trunc + 2.0 ** -54 + 2.0 ** -63 + 4 * 2.0 ** -65 + _hu(L) + _hu(L) + np.abs(e - 1023) * 2.0 ** -54
            + _hu(1023 * math.log(2.0)) + _hu((np.abs(e - 1023) + 1) * math.log(2.0)))


def r2logr2_bound(d2):
    """Bound on |r2logr2(d2) - d2 log d2|: d2 times log_bound (the factor d2 is exact), and the product's rounding"""
    return d2 * log_bound(d2) + _hu(d2 * (np.abs(np.log(d2)) + 1e-12))


EXP_XMAX = 0.5 * math.log(2.0) / 4096.0


def exp_bound(u):
    """Bound on |table_exp_neg_acc(u, 0) / exp(-700 u) - 1| for u in [0, 1], from ensemble.hip.  With y = u NK = k + r,
    |r| <= 1/2 (k is y rounded to nearest: the fma forms y + MAGIC exactly and rounds once), x = r ln 2 / 4096:

      truncation   exp(x) - (1 + x + x^2 / 2) over exp(x): |x|^3 / 6 * exp(2 |x|), |x| <= ln 2 / 8192  (1.01e-13)
      NK           fl(-700 * fl(4096 / LN2_D)): three roundings (the literal, the quotient, the product), each a relative
                   2^-53 at most, on an exponent of 700 u: 700 u * 3 * 2^-53
      r            half an ulp below 1/2, as a share of x: 2^-54 * ln 2 / 4096
      C1, C2       three and five roundings of relative 2^-53 on x and x^2 / 2
      table        2^(j/4096) in [1, 2): half an ulp, relative 2^-53, and exp2l's own error below 2^-63
      q            the second fma of the quadratic: half an ulp at 1 (the first is at 1.7e-4: 2^-66)
      result       the last fma, acc = 0: a relative 2^-53"""
    trunc = EXP_XMAX ** 3 / 6.0 * math.exp(2.0 * EXP_XMAX)
    return (trunc + 700.0 * u * 3 * 2.0 ** -53 + 2.0 ** -54 * EXP_XMAX / 0.5 + (3 * EXP_XMAX + 5 * EXP_XMAX ** 2 / 2) * 2.0 ** -53
            + 2.0 ** -53 + 2.0 ** -63 + 2.0 ** -53 + 2.0 ** -66 + 2.0 ** -53)


@functools.lru_cache(maxsize=None)
def measured():
    """Everything the tests below assert on, computed once; also writes the record."""
    out = {}
    xs = R.log_sweep_points()
    d2 = [float(x) * float(x) for x in xs]
    out["log_d2"] = d2
    norm = [d for d in d2 if d >= 2.0 ** -1022]
    err = np.array([abs(_log_err(R.table_log_biased(d) + R.LOG_BIAS_D, d)) for d in norm])
    bnd = np.array([log_bound(d) for d in norm])
    ex = np.array([math.frexp(d)[1] - 1 for d in norm])
    out["log"] = (np.array(norm), ex, err, bnd)
    perr = np.array([abs(float(_prod_err(d))) for d in norm])
    out["r2logr2"] = (perr, np.array([r2logr2_bound(d) for d in norm]))
    ts = R.exp_sweep_points()
    us = [float(t) * float(t) for t in ts]
    parts = [R.table_exp_neg_acc(min(u, 1.0), 0.0, parts=True) for u in us]
    out["exp_u"], out["exp_parts"] = us, parts
    inr = [(u, p[0]) for u, p in zip(us, parts) if u <= 1.0]
    out["exp"] = (np.array([u for u, _ in inr]), np.array([abs(_exp_relerr(v, u)) for u, v in inr]),
                  np.array([exp_bound(u) for u, _ in inr]))
    far = {}
    for k4 in R.FAR_K4:
        e, ty, kn, c = R.far_layout(k4)
        plan = R.far_plan_choose(kn, e)
        share, fi, ni = R.far_method_error(e, plan, kn, c, 2, 2)
        far[k4] = (plan, ty, share, len(fi), len(ni))
        out.setdefault("far_single", {})[k4] = R.far_single_knot_error(e, plan, kn, 2, 2)
    out["far"] = far
    _write_record(out)
    return out


def _prod_err(d2):
    v = R.r2logr2(d2)
    if mp is not None:
        return mp.mpf(v) - mp.mpf(d2) * mp.log(mp.mpf(d2))
    return R.LD(v) - R.LD(d2) * np.log(R.LD(d2))


def _groups(ex):
    """the sweep by the binade of L = e ln 2 + logc, where the two large roundings happen"""
    L = (ex + 1023) * math.log(2.0)
    return {"L < 512 (d2 < 2^-284)": L < 511.0, "512 <= L < 1024 (2^-284 .. 2^454)": (L >= 512.0) & (L < 1023.0),
            "L >= 1024 (d2 >= 2^455)": L >= 1024.0}


def _write_record(m):
    d, ex, err, bnd = m["log"]
    lines = ["Measured maxima of the host restatements of the device primitives (tests/devmath_ref.py) against " + REF + ",",
             "written by tests/test_devmath_host.py; the bounds are the formulas of that file.", "",
             "table log: |table_log_biased(d2) + LOG_BIAS_D - log d2| over %d arguments, binary exponents -1022 .. 1000" % len(d)]
    for name, sel in _groups(ex).items():
        lines.append("  %-36s measured %.2e   bound %.2e" % (name, err[sel].max(), bnd[sel].max()))
    near1 = (ex >= -60) & (ex <= 300)
    lines.append("  %-36s measured %.2e   bound %.2e" % ("2^-60 <= d2 < 2^301", err[near1].max(), bnd[near1].max()))
    perr, pb = m["r2logr2"]
    lines.append("  r2logr2 against d2 log d2, as a share of its bound (d2 * log bound + half an ulp): %.2f" % (perr / pb).max())
    u, rel, eb = m["exp"]
    lines += ["", "table exp: |table_exp_neg_acc(u, 0) / exp(-700 u) - 1| over %d arguments in [0, 1]" % len(u),
              "  %-36s measured %.2e   bound %.2e" % ("u <= 1/64", rel[u <= 1 / 64].max(), eb[u <= 1 / 64].max()),
              "  %-36s measured %.2e   bound %.2e" % ("all", rel.max(), eb.max()), "",
              "far-field rule: the 16 x 16 Chebyshev interpolant in long double against the exact sum on the centre tile of",
              "devmath_ref.far_layout, as a share of sum_j |c_j phi_j| over the tile's far knots"]
    for k4, (plan, ty, share, nf, nn) in m["far"].items():
        lines.append("  4 * aspect %-5g tile 64 x %-3d aspect %.4f   %d far knots   method error %.2e"
                     % (k4, plan["ty"], plan["tile_aspect"], nf, share))
        lines.append("  %-16s the worst far knot alone, as a share of its own max |phi| on the tile   %.2e" % ("", m["far_single"][k4]))
    try:
        with open(RECORD, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:              # a read-only checkout keeps the committed record
        pass


# ------------------------------------------------------------------------------------------------- coverage --
def test_log_sweep_covers_every_bin_edge_and_exponent():
    d2 = np.array(measured()["log_d2"])
    assert 15000 < d2.size < 25000
    m, ex = np.frexp(d2[d2 >= 2.0 ** -1022])
    m, ex = 2.0 * m, ex - 1
    assert set(range(-1022, 1001)) <= set(ex.tolist())
    b = np.floor((m - 1.0) * R.LOG_TAB_N).astype(int)
    for i in range(R.LOG_TAB_N):
        lo, up = 1.0 + i / R.LOG_TAB_N, 1.0 + (i + 1) / R.LOG_TAB_N
        mi = m[b == i]
        assert ((mi - lo) / lo <= 2.0 ** -20).any(), i
        assert ((up - mi) / up <= 2.0 ** -20).any(), i
        assert (np.abs(mi - 0.5 * (lo + up)) <= 0.125 / R.LOG_TAB_N).any(), i
    # the bin the restatement reads off the high word is the bin of the mantissa
    for d in d2[:3 * R.LOG_TAB_N:7]:
        assert R.log_bin(float(d))[1] == int((float(d) - 1.0) * R.LOG_TAB_N)
    assert (d2 == 0.0).sum() == 0 and (d2 < 2.0 ** -1022).sum() < 20


def test_exp_sweep_covers_every_entry_and_exponent():
    m = measured()
    hit = np.zeros((R.EXP_TAB_N, 3), dtype=bool)
    es = set()
    for u, (v, e, j, r) in zip(m["exp_u"], m["exp_parts"]):
        if u > 1.0:
            continue
        es.add(e)
        for n, r0 in enumerate((-0.5, 0.0, 0.5)):
            hit[j, n] |= abs(r - r0) <= 1e-3
    assert hit.all(), np.argwhere(~hit)[:5]
    assert set(range(0, -1011, -1)) <= es
    us = np.array(m["exp_u"])
    assert (us == 0.0).any() and (us == 1.0).any() and (us > 1.0).sum() >= 3


# ---------------------------------------------------------------------------------------- tables and bounds --
def test_tables_are_the_rounded_values():
    """build_log_table and the exp table against the reference: invc within an ulp of 1 / c, logc = -log(invc) and
    2^(j/4096) within half an ulp and 2^-63 (two roundings, long double then double)."""
    tx, ty = R.log_table()
    et = R.exp_table()
    for i in range(0, R.LOG_TAB_N, 1):
        invc = math.ldexp(float(tx[i]), -1023)
        c = 1.0 + (i + 0.5) / R.LOG_TAB_N
        assert abs(invc * c - 1.0) <= 2.0 ** -52
        assert abs(_log_err(-float(ty[i]), invc)) <= 0.5 * math.ulp(float(ty[i])) + 2.0 ** -63, i
    for j in range(R.EXP_TAB_N):
        want = mp.power(2, mp.mpf(j) / 4096) if mp is not None else np.exp2(R.LD(j) / R.LD(4096.0))
        assert abs(float(want - float(et[j]))) <= 2.0 ** -53 + 2.0 ** -63, j
    assert et[0] == 1.0 and float(tx[0]) == math.ldexp(float(np.float64(R.LD(1.0) / (R.LD(1.0) + R.LD(0.5) / R.LD(1024)))), 1023)


def test_table_log_lies_under_its_derived_bound():
    d, ex, err, bnd = measured()["log"]
    assert (err <= bnd).all(), (d[err > bnd][:5], err[err > bnd][:5])
    for name, sel in _groups(ex).items():
        assert sel.sum() > 1000
        assert 0.1 * bnd[sel].max() <= err[sel].max() <= bnd[sel].max(), (name, err[sel].max(), bnd[sel].max())
    # near d2 = 1 the bound is 1.85e-13, nine times the 2e-14 of log m alone
    near1 = (ex >= -2) & (ex <= 1)
    assert 1.8e-13 < bnd[near1].max() < 1.9e-13
    perr, pb = measured()["r2logr2"]
    assert (perr <= pb).all() and (perr / pb).max() >= 0.1


def test_table_log_special_arguments():
    assert R.r2logr2(0.0) == 0.0
    for d in (5e-324, 2.0 ** -1040, 2.0 ** -1023 * 1.5):
        v = R.r2logr2(d)
        assert math.isfinite(v) and abs(v) < 1e-300


def test_table_exp_lies_under_its_derived_bound():
    u, rel, bnd = measured()["exp"]
    assert (rel <= bnd).all(), (u[rel > bnd][:5], rel[rel > bnd][:5])
    assert 0.1 * bnd.max() <= rel.max() <= bnd.max(), (rel.max(), bnd.max())
    lowu = u <= 1.0 / 64                 # truncation alone: the r = +-1/2 arguments sit right under it
    assert 0.1 * bnd[lowu].max() <= rel[lowu].max() <= bnd[lowu].max()
    # arguments beyond 1 are clamped by the caller; at the clamp the result is exp(-700)
    assert abs(_exp_relerr(R.table_exp_neg_acc(1.0), 1.0)) <= exp_bound(1.0)
    assert R.table_exp_neg_acc(0.0) == 1.0


def test_svr_restatement_matches_the_kernel_formula():
    """svr_predict (the record of mhs_svr_load, the fma chain, the clamp, the two sums) against kernlab's formula in
    long double: sum_i alpha_i exp(-sigma |x - sv_i|^2) - b, scaled back."""
    rng = np.random.default_rng(3)
    sv = rng.normal(0, 0.5, (5, 3))
    alpha = np.array([0.7, -1.3, 0.2, -0.05, 1.0])
    X = rng.normal(0, 1.0, (40, 3)) * [2.0, 0.5, 3.0] + [1.0, -2.0, 0.5]
    xc, xs = np.array([1.0, -2.0, 0.5]), np.array([2.0, 0.5, 3.0])
    got = R.svr_predict(alpha, sv, 0.3, 1.7, xc, xs, 10.0, 2.5, X)
    Z = ((X - xc) / xs).astype(R.LD)
    k = np.exp(-R.LD(1.7) * ((Z[:, None, :] - sv.astype(R.LD)[None]) ** 2).sum(-1))
    want = ((k * alpha.astype(R.LD)).sum(1) - R.LD(0.3)) * R.LD(2.5) + R.LD(10.0)
    assert np.abs(got - want.astype(np.float64)).max() <= 1e-12 * 2.5 * np.abs(alpha).sum()


# ------------------------------------------------------------------------------------------- far-field rule --
@pytest.mark.parametrize("k4,ty,aspect", [(4.0, 64, 1.0), (2.49, 32, 1.245), (2.51, 48, 16 * 2.51 / 48)])
def test_far_layout_is_the_worst_accepted_geometry(k4, ty, aspect):
    plan, ty_l, share, nfar, nnear = measured()["far"][k4]
    e, _, kn, c = R.far_layout(k4)
    assert (plan["tx"], plan["ty"], plan["ntx"], plan["nty"]) == (64, ty, 5, 5) and ty_l == ty
    assert abs(plan["tile_aspect"] - aspect) < 1e-12 and 0.8 <= plan["tile_aspect"] <= 1.25
    assert len(kn) >= 32 and (c > 0).all()
    b, start, order = R.far_plan_sort(plan)
    bx, by = b % 9 - 2, b // 9 - 2
    ring = np.maximum(np.abs(bx - 2), np.abs(by - 2)) == 2
    assert ring.sum() >= 32 and nfar >= 32 and nnear >= 4
    kc, kr = plan["kc"], plan["kr"]
    # the ring's knots lie within one cell of the edge that faces the centre tile
    d = np.minimum.reduce([np.abs(kc - 64), np.abs(kc - 256), np.abs(kr - ty), np.abs(kr - 4 * ty)])
    assert (d[ring] <= 1.0).all()
    assert (kc == 256.0).sum() >= 5 and (kr == 4.0 * ty).sum() >= 5 and (kc == 64.0).sum() >= 2       # exactly on a bin edge
    assert ((kc < -128) | (kc >= 320 + 128) | (kr < -2 * ty) | (kr >= 7 * ty)).sum() >= 4             # collapsed onto the rim
    assert (bx >= -2).all() and (bx <= 6).all() and (by >= -2).all() and (by <= 6).all()
    assert start[-1] == len(kn) and sorted(order.tolist()) == list(range(len(kn)))


def test_far_field_method_error_is_small_at_every_accepted_aspect():
    """1e-10 of the far knots' sum is what far_plan_choose's aspect window has to keep (and the square tile is far
    better than the window's ends)."""
    far = measured()["far"]
    for k4, (plan, ty, share, nfar, nnear) in far.items():
        assert share <= 1e-10, (k4, share)
    assert far[4.0][2] < far[2.49][2] and far[4.0][2] < far[2.51][2]


def test_cheb_matrix_reproduces_polynomials_and_its_lebesgue_constant():
    t = R.cheb_points()
    for cells, flip in ((64, False), (32, True), (48, True)):
        L = R.cheb_matrix(cells, flip, t)
        tau = (2.0 * np.arange(cells) + 1.0) / cells - 1.0
        tau = -tau if flip else tau
        assert np.abs(L.sum(1) - 1.0).max() < 1e-14
        for deg in (1, 5, 15):
            assert np.abs(L @ np.array(t) ** deg - tau ** deg).max() < 1e-13
        assert 1.5 < np.abs(L).sum(1).max() < 2.35            # 2.29 over the whole interval
        assert np.abs(L - R.cheb_matrix(cells, flip, [np.cos(R.LD(2 * a + 1) * R.LD(np.pi) / R.LD(32)) for a in range(16)],
                                        R.LD).astype(np.float64)).max() < 1e-13


def test_the_record_holds_what_was_measured():
    measured()
    text = open(RECORD).read()
    assert "table log" in text and "table exp" in text and "far-field rule" in text and "4 * aspect 2.49" in text
