"""GPU: the proximity entry of the R .Call() shim (mhsr_proximity -> the host entry point mhs_proximity on double planes with the
layout of terra::values), executed through the stand-in R runtime of tests/rstub, equals the Python call on device planes and
the restatement (tests/proximity_ref.py) bit for bit.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import proximity_ref as pr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
ALL = ("d2", "index", "dist", "dir_x", "dir_y", "value")


def test_shim_proximity_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    from machisplin_amd import Geometry
    from machisplin_amd.proximity import proximity
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)
    rng = np.random.default_rng(12)
    z = np.stack([rng.integers(0, 60, (45, 77)).astype(np.float64), np.round(rng.standard_normal((45, 77)), 2)])
    z[0, rng.integers(0, 45, 40), rng.integers(0, 77, 40)] = np.nan                    # NA_real_ cells
    z[0, 20:24, 30:37] = -9999.0                                                       # ... and a nodata value
    z[1, rng.random((45, 77)) < 0.2] = np.nan
    stack = hip.RasterStack(g, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    for code, (where, thr) in enumerate((("na", None), ("valid", None), ("lt", 2.0), ("le", 2.0), ("gt", 57.0), ("ge", 57.0), ("eq", 5.0),
                                         ("ne", 5.0))):
        want, want_info = proximity(stack, 0, where, thr, ALL, value_layer=1, unit=2.5)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        ref = pr.proximity(z[0], -9999.0, where, thr, unit=2.5, value_plane=z[1])
        out = R.values(R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([-9999.0]), R.num([0, code, thr or 0.0, 1, 2.5]), R.int([63])))
        assert len(out) == 7
        for k, name in enumerate(ALL):
            v = R.values(out[k]).reshape(45, 77)
            if name == "index":
                v = v - 1                                                              # a terra cell number
            assert v.dtype == want[name].dtype and np.array_equal(v, want[name], equal_nan=True), (where, name)
            assert np.array_equal(v, ref[name], equal_nan=True), (where, name)
        assert list(R.values(out[6])) == [want_info["n_features"], want_info["max_d2"]]
    # a subset: the planes not asked for are NULL; one layer as a plain vector; value_layer is not looked at
    out = R.values(R.call("mhsr_proximity", R.geom(g), R.num(z[0]), R.num([np.nan]), R.num([0, 0, 0.0, -1, 30.0]), R.int([4])))
    assert all(out[k] == R.NULL for k in (0, 1, 3, 4, 5))
    assert np.array_equal(R.values(out[2]).reshape(45, 77), pr.proximity(z[0], None, "na", unit=30.0)["dist"])
    # no feature anywhere: NA_integer_ and NaN, and the call succeeds
    out = R.values(R.call("mhsr_proximity", R.geom(g), R.num(np.ones(45 * 77)), R.num([np.nan]), R.num([0, 0, 0.0, -1, 30.0]), R.int([7])))
    assert (R.values(out[0]) == NA_INTEGER).all() and (R.values(out[1]) == NA_INTEGER).all() and np.isnan(R.values(out[2])).all()
    assert list(R.values(out[6])) == [0.0, -1.0]
    # refusals of the library and of the shim come back as R errors
    with pytest.raises(RuntimeError, match="unit"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 1, 0.0]), R.int([63]))
    with pytest.raises(RuntimeError, match="value_layer"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 2, 1.0]), R.int([32]))
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([2, 0, 0.0, 1, 1.0]), R.int([4]))
    with pytest.raises(RuntimeError, match=r"\(nrow - 1\)\^2"):
        R.call("mhsr_proximity", R.geom(Geometry(0.0, 1.0, 1.0, 1.0, 1, 50000)), R.num(np.zeros(50000)), R.num([np.nan]),
               R.num([0, 0, 0.0, -1, 1.0]), R.int([4]))
    with pytest.raises(RuntimeError, match="bit mask"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 1, 1.0]), R.int([64]))
    with pytest.raises(RuntimeError, match="where must be"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1.0]), R.int([4]))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 1]), R.int([4]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_proximity", R.geom(g), R.mat(values[:-1]), R.num([np.nan]), R.num([0, 0, 0.0, 1, 1.0]), R.int([4]))
