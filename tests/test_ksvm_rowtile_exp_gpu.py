"""GPU: the row-tile ksvm kernel's own table exponential and its launch.

For P <= 5 svr_rt_kernel forms exp(-700 u) from a staged table of 8192 entries (the 4096 entries 2^(j/4096) twice: the byte
offset keeps the lowest bit of the exponent), drops the exponent field onto the entry by one shift-add, and runs in blocks of
8 waves, each wave with its own 192-cell tile.  Larger P keep the 4096-entry table and blocks of 4.

svr_kernel (MHS_SVR_NO_ROWTILE=1) keeps the 4096-entry table and the bit-field form and is the reference: a wave that does not
fold its cells' q must give svr_kernel's bits.  A folding wave is held to 13 roundings of 700 * 2^-53 each, relative to the
cell's value.  tests/test_devmath_gpu.py derives that count for P = 3 and ONE support vector (two fmas with b_k x_k on the
exponent path); the launch tests below apply it unchanged at P = 5 .. 12 (one more fma per further predictor) and to a
difference of two sums, where it is no longer a derived bound but a stretched one: the models keep the negative sum at a few
per cent of the positive one, and the largest figure seen on the device was 1.8e-13 against the bound's 1.0e-12."""
import math

import numpy as np
import pytest

import devmath_ref as R

pytestmark = pytest.mark.gpu

FOLD_BOUND = 13 * 700.0 * 2.0 ** -53      # test_table_exp_row_tile_kernel_against_the_lane_per_cell_kernel
TILE = 192


def _both_kernels(hip, monkeypatch, stack, m):
    got = hip.predict(stack, m).cpu().numpy()
    monkeypatch.setenv("MHS_SVR_NO_ROWTILE", "1")
    try:
        plain = hip.predict(stack, m).cpu().numpy()
    finally:
        monkeypatch.delenv("MHS_SVR_NO_ROWTILE")
    return got, plain


def _compare_tiles(got, plain, q, what):
    """Tile by tile (192 cells of a row): the bits of svr_kernel where the tile's q spread over more than 0.5 (the wave keeps the
    per-pair addition), the folded form's bound relative to the cell's own value elsewhere.  Returns (folded, unfolded)."""
    nrow, ncol = got.shape
    folded = unfolded = 0
    worst = 0.0
    for r in range(nrow):
        for c0 in range(0, ncol, TILE):
            sl = (r, slice(c0, min(c0 + TILE, ncol)))
            spread = q[sl].max() - q[sl].min()
            assert abs(spread - 0.5) > 0.02, (what, r, c0, spread)
            if spread > 0.5:
                unfolded += 1
                assert np.array_equal(got[sl], plain[sl]), (what, r, c0)
            else:
                folded += 1
                rel = np.abs(got[sl] / plain[sl] - 1.0).max()
                worst = max(worst, rel)
                assert rel <= FOLD_BOUND, (what, r, c0, rel, FOLD_BOUND)
    print(f"{what}: {folded} folded tiles (worst {worst:.3e} of the cell, bound {FOLD_BOUND:.3e}), {unfolded} unfolded tiles")
    return folded, unfolded


# ------------------------------------------------------------------ a. every table entry at both exponent parities --
NCOL_A, ROWS_A = 384, 23                    # 46 waves of 190 free cells each >= 8192 + the ends; one more row folds
XC_A, XS_A = [0.0, 0.1875, 1.0], [1.0, 16.0, 16.0]
C_STAR, ZERO_AT, WIDE_AT = 5, 5, 6          # column of the support vector; per wave: the cell with x0 = 0 and the one with x0 = 0.8


J_LO_A = math.ceil(R.EXP_NK + 4096 * 1010)          # the smallest j whose u stays below 1 at e = -1010
LOWEST_A = [(-1010, J_LO_A), (-1010, 4095), (-1009, 0), (-1009, 4095)]


def _targets_a():
    """(e, j) of the sweep: every j at an odd and at an even e + 1023, e cycling through -2 .. -1007; then the two smallest
    exponents the clamp admits (-700 * 4096 / ln 2 = -1010 * 4096 + 464.8) at both ends of their j"""
    out = []
    for j in range(R.EXP_TAB_N):
        base = 2 + 2 * ((37 * j) % 503)
        out.append((-base, j))              # e + 1023 odd
        out.append((-base - 1, j))          # e + 1023 even
    out += LOWEST_A
    return out


def test_every_table_entry_at_both_exponent_parities(hip, monkeypatch):
    """One layer, one support vector, sigma = 700, rows of 384 columns (two waves each).  The support vector sits at x0 = 0 on the
    centre of cell (0, 5); every quantity of that cell's argument is a short dyadic number, so there u comes out as exactly 0.
    For every other cell x0 = sqrt(u_target - (the LONG and LAT part)) puts round(u NK) on the wanted (e, j).  Every wave holds
    a cell with x0 = 0 and one with x0 = 0.8 (q spread 0.64): no wave of rows 0 .. 22 folds, so those rows must carry
    svr_kernel's bits, and every seventh cell the restatement's.  Row 23 folds (proof that the row-tile kernel ran)."""
    nrow = ROWS_A + 1
    g = hip.Geometry(0.0, 1.0, 2.0 ** -10, 2.0 ** -10, nrow, NCOL_A)
    lon, lat = g.x_from_col(np.arange(NCOL_A)), g.y_from_row(np.arange(nrow))
    x1 = (lon - XC_A[1]) / XS_A[1]
    x2 = (lat - XC_A[2]) / XS_A[2]
    sv = [[0.0, float(x1[C_STAR]), float(x2[0])]]
    ends = [math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 1.25, 1e10]        # x0: u just under, at and beyond the clamp
    targets = _targets_a()
    plane = np.full((nrow, NCOL_A), 0.5)
    slots = [(r, c) for r in range(ROWS_A) for c in range(NCOL_A) if c % TILE not in (ZERO_AT, WIDE_AT)]
    assert len(slots) >= len(targets) + len(ends)
    for (r, c), (e, j) in zip(slots, targets):
        rest = (x1[c] - sv[0][1]) ** 2 + (x2[r] - sv[0][2]) ** 2
        plane[r, c] = math.sqrt((4096 * e + j) / R.EXP_NK - rest)
    for (r, c), x0 in zip(slots[len(targets):], ends):
        rest = (x1[c] - sv[0][1]) ** 2 + (x2[r] - sv[0][2]) ** 2
        plane[r, c] = math.sqrt(x0 - rest) if x0 < 1.0 else x0      # u itself just under 1; u >= 1 with any x0 >= 1
    plane[:ROWS_A, ZERO_AT::TILE] = 0.0
    plane[:ROWS_A, WIDE_AT::TILE] = 0.8
    plane[ROWS_A] = np.random.default_rng(3).uniform(0.3, 0.6, NCOL_A)
    stack = hip.RasterStack(g, plane[None].copy(), float("nan"))
    m = hip.models.Ksvm([1.0], sv, 0.0, 700.0, XC_A, XS_A, 0.0, 1.0)
    got, plain = _both_kernels(hip, monkeypatch, stack, m)

    # what the cells ask of the table, by the restatement: all 8192 (entry, parity) pairs, u = 0, u = 1
    rec, npos, amax = R.svr_record([1.0], sv, 700.0)
    X = np.column_stack([plane.ravel(), np.tile(lon, nrow), np.repeat(lat, NCOL_A)])
    hit, us = set(), []
    for row in X[:ROWS_A * NCOL_A]:
        x, q = [], 0.0
        for k in range(3):
            x.append((float(row[k]) - XC_A[k]) / XS_A[k])
            q = R.fma(x[k], x[k], q)
        u = R.svr_argument(rec[0], x, (700.0 / R.EXP_RANGE) * q)
        _, e, j, _ = R.table_exp_neg_acc(u, parts=True)
        hit.add(((e + 1023) & 1, j))
        us.append((u, e, j))
    assert len(hit) == 2 * R.EXP_TAB_N, len(hit)
    assert us[C_STAR][0] == 0.0 and us[C_STAR][1:] == (0, 0)
    assert sum(u == 1.0 for u, _, _ in us) >= 4 and any(0.999999 < u < 1.0 for u, _, _ in us)
    exps = {e for _, e, _ in us}
    assert J_LO_A == 465 and min(exps) == -1010 and set(LOWEST_A) <= {(e, j) for _, e, j in us}

    Z = (X - XC_A) / XS_A
    q = (Z * Z).sum(1).reshape(nrow, NCOL_A)
    folded, unfolded = _compare_tiles(got, plain, q, "table sweep")
    assert (folded, unfolded) == (2, 2 * ROWS_A)
    assert np.array_equal(got[:ROWS_A], plain[:ROWS_A])
    assert not np.array_equal(got[ROWS_A], plain[ROWS_A])                     # the row-tile kernel did run
    assert got[0, C_STAR] == 1.0
    sub = np.arange(0, ROWS_A * NCOL_A, 7)
    want = R.svr_predict([1.0], sv, 0.0, 700.0, XC_A, XS_A, 0.0, 1.0, X[sub])
    bad = np.flatnonzero(got.ravel()[sub] != want)
    assert bad.size == 0, (bad.size, sub[bad[:5]], got.ravel()[sub][bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------- b, c. the launch: block edges, every P --
def _model_and_stack(hip, P, nrow, ncol, n_pos, n_neg, wide_tiles, seed):
    """P - 2 float64 layers in (-1, 1) and a ksvm model of n_pos + n_neg support vectors clustered around the scaled
    origin, sigma = 0.1: every kernel value lies between 0.05 and 1 and the negative coefficients are small, so a cell's
    value is its positive sum less a few per cent.  In the tiles of `wide_tiles` (row, tile) one cell of layer 0 is 450:
    q = (0.1 / 700) 300^2 there, far more than 0.5 above its neighbours', so that wave does not fold."""
    C = P - 2
    rng = np.random.default_rng(seed)
    g = hip.Geometry(0.0, 1.0, 2.0 ** -10, 2.0 ** -10, nrow, ncol)
    planes = rng.uniform(-1.0, 1.0, (C, nrow, ncol))
    for r, t in wide_tiles:
        planes[0, r, min(t * TILE + 17, ncol - 1)] = 450.0
    xc = list(rng.uniform(-0.2, 0.2, C)) + [ncol * 2.0 ** -11, 1.0 - nrow * 2.0 ** -11]
    xs = list(rng.uniform(0.75, 1.5, C)) + [ncol * 2.0 ** -11, nrow * 2.0 ** -11]          # LONG and LAT scaled to (-1, 1)
    sv = rng.uniform(-0.3, 0.3, (n_pos + n_neg, P))
    alpha = np.concatenate([rng.uniform(0.2, 1.0, n_pos), -rng.uniform(0.01, 0.1, n_neg)])
    order = rng.permutation(n_pos + n_neg)                                                  # the loader sorts by sign
    sigma = 0.1
    m = hip.models.Ksvm(list(alpha[order]), sv[order].tolist(), 0.0, sigma, xc, xs, 0.0, 1.0)
    stack = hip.RasterStack(g, planes.copy(), float("nan"))
    lon, lat = g.x_from_col(np.arange(ncol)), g.y_from_row(np.arange(nrow))
    X = np.column_stack([planes.reshape(C, -1).T, np.tile(lon, nrow), np.repeat(lat, ncol)])
    Z = (X - xc) / xs
    q = (sigma / 700.0) * (Z * Z).sum(1).reshape(nrow, ncol)
    return stack, m, q


def _run(hip, monkeypatch, P, nrow, ncol, n_pos, n_neg, wide_tiles, seed):
    stack, m, q = _model_and_stack(hip, P, nrow, ncol, n_pos, n_neg, wide_tiles, seed)
    got, plain = _both_kernels(hip, monkeypatch, stack, m)
    assert np.isfinite(plain).all() and (plain > 0).all()
    what = f"P={P} {ncol}x{nrow} nsv={n_pos}+{n_neg}"
    folded, unfolded = _compare_tiles(got, plain, q, what)
    assert unfolded == len(wide_tiles) and folded >= 1
    assert not np.array_equal(got, plain), "the row-tile kernel did not run (identical planes)"


@pytest.mark.parametrize("ncol,nrow,n_pos,n_neg,wide", [
    (192, 5, 4, 3, [(1, 0), (4, 0)]),                 # fewer tiles than one block's waves
    (192, 17, 4, 3, [(0, 0), (7, 0), (8, 0), (16, 0)]),     # two blocks and one tile more, alone in the third
    (180, 3, 4, 3, [(2, 0)]),                         # 12 padded lanes at the row end (180 >= 0.93 * 192 keeps the row-tile path)
    (384, 2, 129, 2, [(0, 1)]),                       # 131 support vectors: the positive range crosses the 128-vector chunk
])
def test_block_edges_of_the_row_tile_launch(hip, monkeypatch, ncol, nrow, n_pos, n_neg, wide):
    """P = 5 (blocks of 8 waves, a tile per wave), support vectors of both signs"""
    _run(hip, monkeypatch, 5, nrow, ncol, n_pos, n_neg, wide, seed=ncol + nrow)


@pytest.mark.parametrize("p", [3, 5, 7, 12])
def test_one_predictor_count_of_each_block_shape(hip, monkeypatch, p):
    """4 x 192 cells: P = 3 and 5 run the new exponential in blocks of 8 waves; 7 (three waves per SIMD) and 12 (two) keep the
    4096-entry table and blocks of 4 -- code this file's change leaves as it was, here so that a later change of
    svr_rt_tab2 / svr_rt_waves (csrc/ensemble.hip) meets a test at every shape class"""
    _run(hip, monkeypatch, p, 4, 192, 4, 3, [(1, 0)], seed=100 + p)
