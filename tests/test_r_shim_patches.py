"""GPU: the patches entry of the R .Call() shim (mhsr_patches -> the host entry point mhs_patches on double planes with the
layout of terra::values), executed through the stand-in R runtime of tests/rstub, equals the Python call on device planes and
the restatement (tests/patches_ref.py) exactly.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import patches_ref as pr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
ALL = pr.PRODUCTS


def test_shim_patches_equals_the_device_call_exactly(R, hip):  # noqa: F811
    from machisplin_amd import Geometry
    from machisplin_amd.patches import patches
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)                                   # two tiles side by side, two above each other
    rng = np.random.default_rng(12)
    z = np.stack([rng.integers(0, 60, (45, 77)).astype(np.float64), np.round(rng.standard_normal((45, 77)), 2)])
    z[0, rng.integers(0, 45, 400), rng.integers(0, 77, 400)] = np.nan                  # NA_real_ cells
    z[0, 20:24, 30:37] = -9999.0                                                       # ... and a nodata value
    stack = hip.RasterStack(g, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    cases = ((0, "na", None, 8, 1, None, "any"), (1, "valid", None, 4, 2, 3000, "touching"), (3, "le", 24.0, 8, 3, 40, "interior"),
             (5, "ge", 24.0, 4, 1, 1, "any"), (7, "ne", 5.0, 8, 5, None, "touching"))
    for code, where, thr, conn, lo, hi, edge in cases:
        want, want_info = patches(stack, 0, where, thr, conn, ALL, lo, hi, edge)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        ref, ref_info = pr.patches(pr.features(z[0], -9999.0, where, thr), conn, lo, hi, edge)
        opts = R.num([0, code, thr or 0.0, conn, lo, np.nan if hi is None else hi, pr.EDGE.index(edge)])
        out = R.values(R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([-9999.0]), opts, R.int([31])))
        assert len(out) == 6
        for k, name in enumerate(ALL):
            v = R.values(out[k]).reshape(45, 77)
            assert v.dtype == np.int32
            if name == "label":
                assert ((v == NA_INTEGER) == (ref[name] < 0)).all()
                v = np.where(v == NA_INTEGER, -1, v - 1)                               # a terra cell number
            assert np.array_equal(v, want[name]) and np.array_equal(v, ref[name]), (where, name)
        assert list(R.values(out[5])) == [want_info[k] for k in ("n_features", "n_patches", "n_kept_patches", "n_kept_cells", "max_size")]
        assert list(R.values(out[5])) == [ref_info[k] for k in ("n_features", "n_patches", "n_kept_patches", "n_kept_cells", "max_size")]
    # a subset: the planes not asked for are NULL; one layer as a plain vector; max_size Inf
    out = R.values(R.call("mhsr_patches", R.geom(g), R.num(z[0]), R.num([np.nan]), R.num([0, 0, 0.0, 8, 2, np.inf, 0]), R.int([16 | 2])))
    assert all(out[k] == R.NULL for k in (0, 2, 3))
    ref, _ = pr.patches(np.isnan(z[0]), 8, 2)
    assert np.array_equal(R.values(out[4]).reshape(45, 77), ref["keep"]) and np.array_equal(R.values(out[1]).reshape(45, 77), ref["id"])
    # no feature anywhere: NA_integer_ labels, zeros, and the call succeeds
    out = R.values(R.call("mhsr_patches", R.geom(g), R.num(np.ones(45 * 77)), R.num([np.nan]), R.num([0, 0, 0.0, 8, 1, np.nan, 0]), R.int([31])))
    assert (R.values(out[0]) == NA_INTEGER).all() and all((R.values(out[k]) == 0).all() for k in (1, 2, 3, 4))
    assert list(R.values(out[5])) == [0.0, 0.0, 0.0, 0.0, 0.0]
    # refusals of the library and of the shim come back as R errors
    with pytest.raises(RuntimeError, match="connectivity"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 6, 1, np.nan, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="min_size"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 8, 0, np.nan, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="max_size"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 8, 5, 4, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="edge_rule"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 8, 1, np.nan, 3]), R.int([1]))
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([2, 0, 0.0, 8, 1, np.nan, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="threshold"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 3, np.nan, 8, 1, np.nan, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="bit mask"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 8, 1, np.nan, 0]), R.int([32]))
    with pytest.raises(RuntimeError, match="where must be"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 8, 1, np.nan, 0]), R.int([1]))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_patches", R.geom(g), R.mat(values), R.num([np.nan]), R.num([0, 0, 0.0, 8, 1]), R.int([1]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_patches", R.geom(g), R.mat(values[:-1]), R.num([np.nan]), R.num([0, 0, 0.0, 8, 1, np.nan, 0]), R.int([1]))
