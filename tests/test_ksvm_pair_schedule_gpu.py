"""The hand-scheduled support-vector loop of the resident ksvm kernel at P = 5 (csrc/svr_rt_loop5.inc, svr_rt_loop5q.inc,
written by tools/gen_svr_rt_asm.py) against the compiler's loop it replaces, which MHS_SVR_CXX_LOOP=1 keeps reachable.

The two loops perform the same operations on the same values in the same order; only where the operands come from (the
support-vector coefficients through the wave's LDS slice instead of the scalar cache) and when the instructions issue
(counted lgkmcnt waits) differ.  So every comparison between them is np.array_equal: there is no tolerance.  A wrong wait
count, a wrong offset into the slice or a wrong prologue / epilogue gives other bits, not a fault.

A chunk of n support vectors of one sign (n <= 128) runs (n - 1) >> 2 pipelined trips of four and then 1 .. 4 vectors in
the simple form; the (nsv, npos) below give positive and negative ranges of 1, 2, 3, 4, 5, 7 and 8 vectors, 127 / 128 /
129 / 131 across the chunk boundary, and two full chunks.  Shape: 5 rows of at most 2 817 columns (kc.planes: an all-NA
tile, NA cells in a last tile, a wave that does not fold, one live lane in the row's last tile at 2 689)."""
import os

import numpy as np
import pytest

import ksvm_resident_cases as kc
from oracle import ensemble as oe

pytestmark = pytest.mark.gpu

SV_COUNTS = [(2, 1), (5, 1), (5, 4), (8, 4), (9, 5), (12, 7), (37, None), (131, 129), (131, 2), (256, 128), (259, 129),
             (262, 131), (300, 150)]


def _with_env(name, fn):
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def _both(hip, geom, pl, nodata, prm):
    hand = kc.row_tile_plane(hip, geom, pl, nodata, prm)
    cxx = _with_env("MHS_SVR_CXX_LOOP", lambda: kc.row_tile_plane(hip, geom, pl, nodata, prm))
    return hand, cxx


def _narrow(prm, C):
    """The p = 5 model of kc.svr_params on C covariates, LONG and LAT: p = C + 2."""
    keep = list(range(C)) + [3, 4]
    out = dict(prm)
    out["sv"] = prm["sv"][:, keep]
    out["x_center"] = prm["x_center"][keep]
    out["x_scale"] = prm["x_scale"][keep]
    return out


@pytest.mark.parametrize("nsv,npos", SV_COUNTS)
@pytest.mark.parametrize("ncol", [2689, 2753])
def test_hand_loop_equals_the_compilers_loop_bit_for_bit(hip, ncol, nsv, npos):
    """2 689: one live lane in the row's last tile; the only wave that does not fold there is the all-NA tile's, whose plane
    is NaN whatever the loop does.  2 753 (65 live columns) has the spike's three cells and ordinary ones in one wave of row
    3, so the loop that keeps q + ap (svr_rt_loop5q.inc) is compared on finite cells at every count as well."""
    from machisplin_amd import synth
    geom = synth.grid(5, ncol)
    pl, nodata = kc.planes(5, ncol)
    prm = kc.svr_params(geom, nsv=nsv, npos=npos)
    assert npos is None or int((prm["alpha"] > 0).sum()) == npos
    hand, cxx = _both(hip, geom, pl, nodata, prm)
    last = ((ncol - 1) // kc.TILE) * kc.TILE
    assert np.isnan(hand[1, 3 * kc.TILE:4 * kc.TILE]).all() and np.isnan(hand[2, ncol - 1]) and not np.isnan(hand[0]).any()
    assert np.isfinite(hand[3, last:]).all()
    assert np.array_equal(hand, cxx, equal_nan=True)


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("ncol", kc.GOLDEN_NCOLS)
def test_widths(hip, ncol, dtype):
    """192, 1, 65 and 129 live columns in a row's last tile, 37 support vectors."""
    from machisplin_amd import synth
    geom = synth.grid(5, ncol)
    pl, nodata = kc.planes(5, ncol, dtype)
    hand, cxx = _both(hip, geom, pl, nodata, kc.svr_params(geom))
    assert np.isnan(hand).any() and np.isfinite(hand).any()
    assert np.array_equal(hand, cxx, equal_nan=True)


@pytest.mark.parametrize("nsv,npos", [(37, None), (131, 129)])
@pytest.mark.parametrize("C", [1, 2])
def test_p3_and_p4_keep_the_compilers_loop(hip, C, nsv, npos):
    """The hand loop is emitted for P = 5 only: at P = 3 and 4 (one and two covariate planes) launch_svr takes the compiler's
    loop with or without the switch, and the switch changes nothing."""
    from machisplin_amd import synth
    geom = synth.grid(5, 2689)
    pl, nodata = kc.planes(5, 2689)
    prm = _narrow(kc.svr_params(geom, nsv=nsv, npos=npos), C)
    pl = np.ascontiguousarray(pl[:C])
    plain, switched = _both(hip, geom, pl, nodata, prm)
    assert np.isfinite(plain).any()
    assert np.array_equal(plain, switched, equal_nan=True)
    X = kc.host_predictors(geom, pl, nodata)
    want = oe.predict(prm, X).reshape(plain.shape)
    assert np.array_equal(np.isnan(plain), np.isnan(want))
    assert np.nanmax(np.abs(plain - want)) <= 1e-11 * np.nanmax(np.abs(want))


def test_against_the_oracle_and_the_lane_per_cell_kernel(hip):
    """(259, 129): two chunks and a rest of one on the positive side, 128 + 2 on the negative.  The tolerances of
    tests/test_ksvm_resident_gpu.py: 1e-11 of the prediction against the oracle, 1e-12 against svr_kernel."""
    from machisplin_amd import synth
    geom = synth.grid(5, 2689)
    pl, nodata = kc.planes(5, 2689)
    prm = kc.svr_params(geom, nsv=259, npos=129)
    hand = kc.row_tile_plane(hip, geom, pl, nodata, prm)
    plain = _with_env("MHS_SVR_NO_ROWTILE", lambda: kc.row_tile_plane(hip, geom, pl, nodata, prm))
    want = oe.predict(prm, kc.host_predictors(geom, pl, nodata)).reshape(hand.shape)
    assert np.array_equal(np.isnan(hand), np.isnan(plain)) and np.array_equal(np.isnan(hand), np.isnan(want))
    assert not np.array_equal(hand, plain, equal_nan=True), "the row-tile kernel did not run (identical planes)"
    assert np.nanmax(np.abs(hand - plain)) <= 1e-12 * np.nanmax(np.abs(plain))
    assert np.nanmax(np.abs(hand - want)) <= 1e-11 * np.nanmax(np.abs(want))


def test_window_of_a_larger_raster_with_accumulate(hip):
    """Rows 1..5, columns 100..2788 of a 9 x 3000 raster with weight 0.7 added into a plane: hand loop and compiler's loop
    leave the same bits, which are emit()'s two operations on the plain window."""
    import torch
    from machisplin_amd import synth
    geom = synth.grid(9, 3000)
    pl, nodata = kc.planes(9, 3000)
    prm = kc.svr_params(geom, nsv=131, npos=129)
    stack = hip.RasterStack(geom, pl, nodata)
    model = hip.models.from_param_dict(prm)
    win = (1, 6, 100, 2789)
    base = np.random.default_rng(1).random((5, 2689))

    def run():
        out = torch.from_numpy(base.copy()).to(stack.planes.device)
        hip.predict(stack, model, window=win, weight=0.7, accumulate=True, out=out)
        return hip.predict(stack, model, window=win).cpu().numpy(), out.cpu().numpy()

    got, acc = run()
    got_cxx, acc_cxx = _with_env("MHS_SVR_CXX_LOOP", run)
    assert np.isnan(got).any() and np.isfinite(got).any()
    assert np.array_equal(got, got_cxx, equal_nan=True) and np.array_equal(acc, acc_cxx, equal_nan=True)
    assert np.array_equal(acc, base + got * 0.7, equal_nan=True)
