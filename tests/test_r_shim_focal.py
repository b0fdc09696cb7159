"""GPU: the focal entry of the R .Call() shim (mhsr_focal -> the host entry point mhs_focal: row bands through the same kernels),
executed through the stand-in R runtime of tests/rstub, equals the direct C call on device planes (focal.focal -> mhs_focal_dev) and
the numpy restatement (tests/focal_ref.py) bit for bit.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import focal_ref as fr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def test_shim_focal_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    from machisplin_amd import Geometry, focal
    R.call("mhsr_init", R.int([0]))
    g = Geometry(500000.0, 4100000.0, 30.0, 30.0, 75, 140)
    rng = np.random.default_rng(21)
    r, c = np.meshgrid(np.arange(75.0), np.arange(140.0), indexing="ij")
    z = np.stack([1800.0 + 3.0 * r - 1.5 * c + 40.0 * rng.standard_normal((75, 140)) * rng.random((75, 140)), rng.standard_normal((75, 140))])
    z[0, rng.integers(0, 75, 80), rng.integers(0, 140, 80)] = np.nan                   # NA_real_ cells
    z[0, 30] = np.nan                                                                  # an all-NA row
    z[0, 40:44, 50:57] = -9999.0                                                       # ... and a nodata value
    stack = hip.RasterStack(g, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    radii = (2, 65, 140)
    for shape, names in (("square", fr.STATS), ("circle", ("count", "sum", "mean", "sd", "minus_mean", "dev"))):
        mask = sum(1 << fr.STATS.index(k) for k in names)
        for fill in (0, 1):
            want = focal.focal(stack, radii, names, shape=shape, fill_na=bool(fill), offset=1700.0).cpu().numpy()
            got = R.values(R.call("mhsr_focal", R.geom(g), R.mat(values), R.num([-9999.0]), R.num([0, ("square", "circle").index(shape), fill, 1700.0]),
                                  R.int(radii), R.int([mask])))
            assert got.shape == (g.nrow * g.ncol, 3 * len(names))
            got = got.T.reshape(3, len(names), g.nrow, g.ncol)
            assert np.array_equal(got, want, equal_nan=True), (shape, fill)
            for k, Rk in enumerate(radii):
                assert np.array_equal(want[k], fr.focal(z[0], -9999.0, Rk, names, shape, bool(fill), 1700.0), equal_nan=True), (shape, fill, Rk)
            assert np.isnan(want).any() and (~np.isnan(want)).mean() > 0.5
    # the second layer as a plain vector, NA_real_ for "no nodata value" and for "no offset"
    got = R.values(R.call("mhsr_focal", R.geom(g), R.num(z[1]), R.num([np.nan]), R.num([0, 0, 0, np.nan]), R.int([3]), R.int([4 | 8])))
    assert np.array_equal(got.T.reshape(2, g.nrow, g.ncol), fr.focal(z[1], np.nan, 3, ("mean", "sd"), "square", False, 0.0), equal_nan=True)
    # refusals of the library and of the shim come back as R errors
    args = lambda **kw: [kw.get("geom", R.geom(g)), kw.get("planes", R.mat(values)), R.num([np.nan]), R.num(kw.get("opts", [0, 0, 0, 0.0])),
                         kw.get("radii", R.int([3])), R.int([kw.get("mask", 4)])]
    with pytest.raises(RuntimeError, match="radius must be in 1 .. 140"):
        R.call("mhsr_focal", *args(radii=R.int([141])))
    with pytest.raises(RuntimeError, match="radii must be 1 .. 8 integers"):
        R.call("mhsr_focal", *args(radii=R.int(list(range(1, 10)))))
    with pytest.raises(RuntimeError, match="radii must be 1 .. 8 integers"):
        R.call("mhsr_focal", *args(radii=R.num([3.0])))
    with pytest.raises(RuntimeError, match="circle window gives the sum family"):
        R.call("mhsr_focal", *args(opts=[0, 1, 0, 0.0], mask=32))
    with pytest.raises(RuntimeError, match="stats must be a bit mask"):
        R.call("mhsr_focal", *args(mask=4096))
    with pytest.raises(RuntimeError, match="layer 2 is not one of"):
        R.call("mhsr_focal", *args(opts=[2, 0, 0, 0.0]))
    with pytest.raises(RuntimeError, match="shape must be"):
        R.call("mhsr_focal", *args(opts=[0, 2, 0, 0.0]))
    with pytest.raises(RuntimeError, match="offset must be finite"):
        R.call("mhsr_focal", *args(opts=[0, 0, 0, np.inf]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_focal", *args(planes=R.mat(values[:-1])))
