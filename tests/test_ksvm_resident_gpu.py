"""The ksvm row-tile kernel with resident waves (a wave pulls tile after tile from a device-side counter): every plane is,
bit for bit, the plane of the one-tile-per-wave kernel it replaces (tests/golden/ksvm_rowtile_parent.npz, recorded by
tools/make_ksvm_rowtile_golden.py from a build of the commit before), agrees with the lane-per-cell kernel to 1e-12 and
with the oracle to 1e-11 of the prediction (the tolerances of test_ksvm_row_tile_kernel_alone_matches_the_oracle), and
does not depend on what else is in flight.

Shapes: a tile is 192 columns.  2688 = 14 tiles, 2689 / 2753 / 2817 leave 1 / 65 / 129 live columns in the 15th (one live
lane; one and two lanes' worth of padded cells); all pass launch_svr's 0.93 rule (2689 / 2880 = 0.934).  The padded lanes
of a row's last tile repeat the row's last column, as they always did: a form that gives such a tile fewer cells per lane
was measured and not kept, and these shapes are what it would have to reproduce."""
import functools
import os

import numpy as np
import pytest

import ksvm_resident_cases as kc
from oracle import ensemble as oe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ksvm_rowtile_parent.npz")


def _tol(ref):
    return 1e-11 * np.nanmax(np.abs(ref))


def _lane_kernel(fn):
    os.environ["MHS_SVR_NO_ROWTILE"] = "1"
    try:
        return fn()
    finally:
        del os.environ["MHS_SVR_NO_ROWTILE"]


def _check_against_lane_kernel_and_oracle(got, plain, want):
    assert np.array_equal(np.isnan(got), np.isnan(plain)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert not np.array_equal(got, plain, equal_nan=True), "the row-tile kernel did not run (identical planes)"
    assert np.nanmax(np.abs(got - plain)) <= 1e-12 * np.nanmax(np.abs(plain))
    assert np.nanmax(np.abs(got - want)) <= _tol(want)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("key,ncol,nsv,npos", kc.golden_cases())
def test_planes_are_the_one_tile_per_wave_kernels_bits(hip, key, ncol, nsv, npos):
    """The 5-row shapes, 37 support vectors (131, 129 of them positive, at the one-live-lane width: a second chunk of the
    128-vector staging), with an all-NA tile in row 1, NA cells inside the last (ragged) tile of row 2 and a last tile in
    row 3 whose q spreads more than 0.5, so that its wave keeps the per-pair addition."""
    from machisplin_amd import synth
    geom = synth.grid(kc.GOLDEN_NROW, ncol)
    pl, nodata = kc.planes(kc.GOLDEN_NROW, ncol, "f32")
    prm = kc.svr_params(geom, nsv=nsv, npos=npos)
    assert str(_golden()[key + "_sha256"]) == kc.digest(pl, prm), "the inputs are not the recorded ones: the fixture says nothing"
    got = kc.row_tile_plane(hip, geom, pl, nodata, prm)
    plain = _lane_kernel(lambda: kc.row_tile_plane(hip, geom, pl, nodata, prm))
    X = kc.host_predictors(geom, pl, nodata)
    want = oe.predict(prm, X).reshape(got.shape)
    _check_against_lane_kernel_and_oracle(got, plain, want)
    last = ((ncol - 1) // kc.TILE) * kc.TILE
    assert np.isnan(got[1, 3 * kc.TILE:4 * kc.TILE]).all() and np.isnan(got[2, ncol - 1]) and not np.isnan(got[0]).any()
    xt = (X - prm["x_center"]) / prm["x_scale"]
    q = (prm["sigma"] / 700.0 * (xt * xt).sum(1)).reshape(got.shape)
    if ncol - last >= 3:          # the spike's three cells and ordinary ones in one wave: no fold, the lane kernel's bits
        assert q[3, last:].max() - q[3, last:].min() > 0.5 and q[0, last:].max() - q[0, last:].min() < 0.5
        assert np.array_equal(got[3, last:], plain[3, last:])
        assert not np.array_equal(got[0, last:], plain[0, last:])
    assert np.array_equal(got, _golden()[key], equal_nan=True)


@pytest.mark.parametrize("nrow", [330, 2])
def test_more_tiles_than_resident_waves_and_fewer_tiles_than_waves(hip, nrow):
    """330 x 2689: 4 950 tiles for the 4 096 waves a 256-unit device holds (one block of sixteen per unit), so waves take a
    second tile.  2 x 2689: 30 tiles; the launch holds no more blocks than cover them (two, 32 waves), and the second
    block's two spare waves find the pool empty behind the staging barrier and leave."""
    from machisplin_amd import synth
    geom = synth.grid(nrow, 2689)
    pl, nodata = kc.planes(nrow, 2689, "f32")
    prm = kc.svr_params(geom)
    got = kc.row_tile_plane(hip, geom, pl, nodata, prm)
    plain = _lane_kernel(lambda: kc.row_tile_plane(hip, geom, pl, nodata, prm))
    want = oe.predict(prm, kc.host_predictors(geom, pl, nodata)).reshape(got.shape)
    _check_against_lane_kernel_and_oracle(got, plain, want)


@pytest.mark.parametrize("dtype", ["f32", "f64", "i16"])
def test_window_of_a_larger_raster_with_accumulate(hip, dtype):
    """Rows 1..5, columns 100..2788 of a 9 x 3000 raster: 2689 columns, so a one-live-lane tile at the window's row ends,
    the window's tiles shifted by 100 against the raster's, and the 192 NA cells of raster row 1 spread over two of them.
    The window's plane against the oracle and the lane kernel, and with accumulate on, out + 0.7 * plane in exactly
    emit()'s two operations."""
    import torch
    from machisplin_amd import synth
    geom = synth.grid(9, 3000)
    pl, nodata = kc.planes(9, 3000, dtype)
    prm = kc.svr_params(geom)
    stack = hip.RasterStack(geom, pl, nodata)
    model = hip.models.from_param_dict(prm)
    win = (1, 6, 100, 2789)
    got = hip.predict(stack, model, window=win).cpu().numpy()
    plain = _lane_kernel(lambda: hip.predict(stack, model, window=win).cpu().numpy())
    want = oe.predict(prm, kc.host_predictors(geom, pl, nodata)).reshape(9, 3000)[1:6, 100:2789]
    assert np.isnan(got).any()
    _check_against_lane_kernel_and_oracle(got, plain, want)
    base = np.random.default_rng(1).random(got.shape)
    out = torch.from_numpy(base).to(stack.planes.device)
    hip.predict(stack, model, window=win, weight=0.7, accumulate=True, out=out)
    assert np.array_equal(out.cpu().numpy(), base + got * 0.7, equal_nan=True)


def test_launches_in_flight_together_do_not_share_a_tile_counter(hip):
    """The same model on two streams at once into two planes (330 x 2689 cells x 2 000 support vectors: about a
    millisecond each, launched microseconds apart), three times over; then 150 launches of a 30-tile window on the two
    streams in turns -- more than twice round the ring of 64 counters, with no host synchronisation in between.  Every plane
    equals the plane of a launch that ran alone, bit for bit: waves that counted in a shared or a half-reset word would
    skip tiles (cells left at the NaN the plane was filled with) or run them twice."""
    import torch
    from machisplin_amd import synth
    geom = synth.grid(330, 2689)
    pl, nodata = kc.planes(330, 2689, "f32")
    prm = kc.svr_params(geom, nsv=2000)
    stack = hip.RasterStack(geom, pl, nodata)
    model = hip.models.from_param_dict(prm)
    alone = hip.predict(stack, model)
    torch.cuda.synchronize()
    dev = stack.planes.device
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for _ in range(3):
        o1 = torch.full((330, 2689), float("nan"), dtype=torch.float64, device=dev)
        o2 = torch.full((330, 2689), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        hip.predict(stack, model, out=o1, stream=s1.cuda_stream)
        hip.predict(stack, model, out=o2, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(o1.nan_to_num(nan=-1e300), alone.nan_to_num(nan=-1e300))
        assert torch.equal(o2.nan_to_num(nan=-1e300), alone.nan_to_num(nan=-1e300))
    win = (7, 9, 0, 2689)
    small = alone[7:9]
    outs = torch.full((150, 2, 2689), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for k in range(150):
        hip.predict(stack, model, window=win, out=outs[k], stream=(s1 if k % 2 == 0 else s2).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(outs.nan_to_num(nan=-1e300), small.nan_to_num(nan=-1e300).expand(150, 2, 2689))
