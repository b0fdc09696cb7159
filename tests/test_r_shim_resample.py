"""GPU: the resample entries of the R .Call() shim (mhsr_resample, mhsr_extract -> the host entry points mhs_resample and
mhs_extract_points on double planes with the layout of terra::values), executed through the stand-in R runtime of tests/rstub,
equal the Python calls on device planes bit for bit -- in one piece and with the target going up in several row bands.  Bad
arguments come back as R errors."""
import numpy as np
import pytest

import resample_ref as rr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def test_shim_resample_entries_equal_the_device_calls_bit_for_bit(R, hip, monkeypatch):  # noqa: F811
    import torch
    from machisplin_amd import Geometry
    from machisplin_amd.resample import extract, resample
    R.call("mhsr_init", R.int([0]))
    S = Geometry(1000.0, 5000.0, 30.0, 28.5, 45, 77)
    rng = np.random.default_rng(12)
    r, c = np.meshgrid(np.arange(45.0), np.arange(77.0), indexing="ij")
    z = np.stack([500.0 + 4.0 * r - 2.0 * c + 20.0 * rng.standard_normal((45, 77)), 10.0 + rng.standard_normal((45, 77))])
    z[0, rng.integers(0, 45, 60), rng.integers(0, 77, 60)] = np.nan                    # NA_real_ cells
    z[1, 20:24, 30:37] = -9999.0                                                       # ... and a nodata value
    stack = hip.RasterStack(S, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    fine = Geometry(S.xmin - 3.3 * 30.0, S.ymax + 2.1 * 28.5, 30.0 / 2.3, 28.5 / 2.3, 120, 190)
    coarse = Geometry(S.xmin + 0.4 * 30.0, S.ymax - 0.2 * 28.5, 3.7 * 30.0, 3.7 * 28.5, 13, 21)
    for bands in (None, "4"):
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)
        for T, methods in ((fine, ("near", "bilinear", "cubic")), (coarse, rr.METHODS)):
            for method in methods:
                want = resample(stack, T, method, out_dtype=torch.float64).planes.cpu().numpy()
                got = R.values(R.call("mhsr_resample", R.geom(S), R.mat(values), R.num([-9999.0]), R.geom(T), R.int([rr.METHODS.index(method)])))
                assert got.shape == (T.nrow * T.ncol, 2) and np.array_equal(got.T.reshape(2, T.nrow, T.ncol), want, equal_nan=True), (bands, method)
    monkeypatch.delenv("MHS_HOST_BANDS")
    assert np.array_equal(want[0], rr.resample(z[0], -9999.0, S, coarse, "count"))
    # one layer as a plain vector, NA_real_ for "no nodata value"
    got = R.values(R.call("mhsr_resample", R.geom(S), R.num(z[0]), R.num([np.nan]), R.geom(coarse), R.int([3])))
    assert np.array_equal(got.reshape(coarse.nrow, coarse.ncol), rr.resample(z[0], np.nan, S, coarse, "mean"), equal_nan=True)
    # points
    xy = np.column_stack([rng.uniform(S.xmin - 60.0, S.xmax + 60.0, 300), rng.uniform(S.ymin - 60.0, S.ymax + 60.0, 300)])
    for code, method in enumerate(("simple", "bilinear", "cubic")):
        got = R.values(R.call("mhsr_extract", R.geom(S), R.mat(values), R.num([-9999.0]), R.mat(xy), R.int([code])))
        assert got.shape == (300, 2) and np.array_equal(got, extract(stack, xy, method), equal_nan=True), method
        assert np.isnan(got).any() and (~np.isnan(got)).sum() > 300
    # refusals of the library and of the shim come back as R errors
    with pytest.raises(RuntimeError, match="unknown method"):
        R.call("mhsr_resample", R.geom(S), R.mat(values), R.num([np.nan]), R.geom(coarse), R.int([8]))
    with pytest.raises(RuntimeError, match="aggregate method"):
        R.call("mhsr_extract", R.geom(S), R.mat(values), R.num([np.nan]), R.mat(xy), R.int([3]))
    with pytest.raises(RuntimeError, match="cell size"):
        R.call("mhsr_resample", R.geom(S), R.mat(values), R.num([np.nan]), R.geom(Geometry(0.0, 1.0, 0.0, 1.0, 3, 3)), R.int([1]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_resample", R.geom(S), R.mat(values[:-1]), R.num([np.nan]), R.geom(coarse), R.int([1]))
    with pytest.raises(RuntimeError, match="2 columns"):
        R.call("mhsr_extract", R.geom(S), R.mat(values), R.num([np.nan]), R.mat(np.zeros((5, 3))), R.int([0]))
