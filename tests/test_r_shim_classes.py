"""GPU: the two class entries of the R .Call() shim (mhsr_class_crosstab -> mhs_class_crosstab and mhsr_class_aggregate ->
mhs_class_aggregate, the host entry points on double planes with the layout of terra::values), executed through the stand-in R
runtime of tests/rstub, equal the Python calls on device planes and the restatement (tests/classes_ref.py) exactly.  Bad
arguments come back as R errors."""
import numpy as np
import pytest

import classes_ref as cr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
TABLE = ("counts", "n", "other", "cells", "mode", "mode_frac", "variety", "simpson", "frac")      # the bits of `stats`, in order
PLANES = ("mode", "mode_frac", "variety", "simpson", "n", "frac")                                # the bits of `planes_mask`
PRODUCTS = ("mode", "variety", "n", "mode_frac", "simpson", "frac")                              # the bits of `products`
INFO = ("K", "n_zones", "n_valid", "n_na", "n_other")
CODES = [11, 21, 41, 42, 90]


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _land_cover(shape, seed):
    rng = np.random.default_rng(seed)
    z = np.stack([rng.choice(np.array(CODES + [7], dtype=np.float64), size=shape), rng.choice(np.array([1.0, 2.0, 2.5]), size=shape)])
    z[0, rng.random(shape) < 0.08] = np.nan                                                       # NA_real_ cells
    z[0, 3:6, 4:9] = -9999.0                                                                      # ... and a nodata value
    return z


def test_shim_class_crosstab_equals_the_device_call_exactly(R, hip):  # noqa: F811
    import torch
    from machisplin_amd import Geometry
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)
    z = _land_cover((45, 77), 12)
    rng = np.random.default_rng(13)
    zones = rng.integers(0, 30, (45, 77)).astype(np.int32)
    zones[:, 40:60] = 11
    zones[rng.random((45, 77)) < 0.05] = NA_INTEGER                                               # NA_integer_: no zone
    zones[3, 3] = -5
    stack = hip.RasterStack(g, z, -9999.0)
    values = z.reshape(2, -1).T                                                                   # terra::values: ncell x C
    for layer, nz, classes, frac_of in ((0, 31, CODES, (42, 11)), (0, 0, None, ()), (1, 0, [2, 1], ()), (0, 40, [90, 11], (90,))):
        want = cr.crosstab(z[layer], zones, classes, -9999.0, n_zones=nz or None, frac_of=frac_of)
        dt, dp, dinfo = hip.classes.crosstab(stack, torch.from_numpy(zones), layer, classes, nz or None, TABLE, PLANES, frac_of)
        out = R.values(R.call("mhsr_class_crosstab", R.geom(g), R.mat(values), R.num([-9999.0]), R.int(zones), R.num([layer, nz]),
                              R.int(classes) if classes else R.NULL, R.int(frac_of) if frac_of else R.NULL, R.int([511]), R.int([63])))
        assert len(out) == 4
        tab, planes, info, codes = R.values(out[0]), R.values(out[1]), R.values(out[2]), R.values(out[3])
        assert len(tab) == 9 and len(planes) == 6
        for k, name in enumerate(TABLE):
            v = R.values(tab[k])
            if name in ("counts", "frac"):
                v = np.ascontiguousarray(v.T)                                                     # a zone is a column of the shim's matrix
            assert _bits(v, want[0][name]) and _bits(v, dt[name].cpu().numpy()), (layer, name)
        for k, name in enumerate(PLANES):
            v = R.values(planes[k])
            v = np.ascontiguousarray(v.T).reshape(-1, 45, 77) if name == "frac" else v.reshape(45, 77)
            assert _bits(v, want[1][name]) and _bits(v, dp[name].cpu().numpy()), (layer, name)
        assert list(info) == [float(want[2][k]) for k in INFO] == [float(dinfo[k]) for k in INFO]
        assert list(codes) == want[2]["codes"] == dinfo["codes"]
    # a subset: what is not asked for is NULL; one layer as a plain vector; planes only
    want = cr.crosstab(z[0], zones, CODES)
    out = R.values(R.call("mhsr_class_crosstab", R.geom(g), R.num(z[0]), R.num([np.nan]), R.int(zones), R.num([0, 0]), R.int(CODES), R.NULL, R.int([16 | 128]),
                          R.int([2])))
    tab, planes = R.values(out[0]), R.values(out[1])
    assert all(tab[k] == R.NULL for k in (0, 1, 2, 3, 5, 6, 8)) and all(planes[k] == R.NULL for k in (0, 2, 3, 4, 5))
    assert _bits(R.values(tab[4]), want[0]["mode"]) and _bits(R.values(tab[7]), want[0]["simpson"])
    assert _bits(R.values(planes[1]).reshape(45, 77), want[1]["mode_frac"])
    out = R.values(R.call("mhsr_class_crosstab", R.geom(g), R.num(z[0]), R.num([np.nan]), R.int(zones), R.num([0, 0]), R.NULL, R.NULL, R.int([0]), R.int([1])))
    assert all(t == R.NULL for t in R.values(out[0])) and _bits(R.values(R.values(out[1])[0]).reshape(45, 77), cr.crosstab(z[0], zones)[1]["mode"])
    # no zone anywhere: an empty table, -1 / NaN planes, and the call succeeds
    nowhere = np.full((45, 77), NA_INTEGER, dtype=np.int32)
    out = R.values(R.call("mhsr_class_crosstab", R.geom(g), R.num(z[0]), R.num([np.nan]), R.int(nowhere), R.num([0, 0]), R.int(CODES), R.NULL, R.int([2 | 1]),
                          R.int([1 | 8])))
    assert R.values(R.values(out[0])[1]).size == 0 and (R.values(R.values(out[1])[0]) == -1).all() and np.isnan(R.values(R.values(out[1])[3])).all()
    assert list(R.values(out[2]))[:2] == [5.0, 0.0]
    # refusals of the library and of the shim come back as R errors
    args = lambda opts, ts=2, ps=0, zn=zones, pl=None, cl=CODES, fo=None: (R.geom(g), pl if pl is not None else R.mat(values), R.num([np.nan]), R.int(zn),  # noqa: E731
                                                                            R.num(opts), R.int(cl) if cl is not None else R.NULL,
                                                                            R.int(fo) if fo is not None else R.NULL, R.int([ts]), R.int([ps]))
    with pytest.raises(RuntimeError, match="not below n_zones 29"):
        R.call("mhsr_class_crosstab", *args([0, 29]))
    with pytest.raises(RuntimeError, match="twice"):
        R.call("mhsr_class_crosstab", *args([0, 0], cl=[4, 5, 4]))
    with pytest.raises(RuntimeError, match="must be in 0 .. 65535"):
        R.call("mhsr_class_crosstab", *args([0, 0], cl=[4, 65536]))
    with pytest.raises(RuntimeError, match="is not one of the 5 classes"):
        R.call("mhsr_class_crosstab", *args([0, 0], ts=256, fo=[12]))
    with pytest.raises(RuntimeError, match="1 .. 256 codes"):
        R.call("mhsr_class_crosstab", *args([0, 0], cl=list(range(257))))
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_class_crosstab", *args([2, 0]))
    with pytest.raises(RuntimeError, match="no output"):
        R.call("mhsr_class_crosstab", *args([0, 0], ts=0))
    with pytest.raises(RuntimeError, match="stats must be"):
        R.call("mhsr_class_crosstab", *args([0, 0], ts=512))
    with pytest.raises(RuntimeError, match="planes_mask must be"):
        R.call("mhsr_class_crosstab", *args([0, 0], ps=64))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_class_crosstab", *args([0, 0, 0]))
    with pytest.raises(RuntimeError, match="one zone per cell"):
        R.call("mhsr_class_crosstab", *args([0, 0], zn=zones[:-1]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_class_crosstab", *args([0, 0], pl=R.mat(values[:-1])))


def test_shim_class_aggregate_equals_the_device_call_exactly(R, hip):  # noqa: F811
    from machisplin_amd import Geometry
    R.call("mhsr_init", R.int([0]))
    S = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)
    z = _land_cover((45, 77), 14)
    stack = hip.RasterStack(S, z, -9999.0)
    values = z.reshape(2, -1).T
    targets = (Geometry(1000.0, 5000.0, 90.0, 90.0, 15, 26), Geometry(1011.1, 4988.9, 75.0, 75.0, 20, 33), Geometry(1300.0, 4700.0, 12.0, 12.0, 9, 11))
    for T in targets:
        for layer, classes, frac_of in ((0, CODES, (42, 11)), (0, None, ()), (1, [2, 1], ())):
            want, winfo = cr.aggregate(z[layer], S, T, classes, -9999.0, frac_of)
            dp, dinfo = hip.classes.aggregate(stack, T, layer, classes, PRODUCTS, frac_of)
            out = R.values(R.call("mhsr_class_aggregate", R.geom(S), R.mat(values), R.num([-9999.0]), R.geom(T), R.num([layer]),
                                  R.int(classes) if classes else R.NULL, R.int(frac_of) if frac_of else R.NULL, R.int([63])))
            assert len(out) == 3
            planes, info, codes = R.values(out[0]), R.values(out[1]), R.values(out[2])
            for k, name in enumerate(PRODUCTS):
                v = R.values(planes[k])
                v = np.ascontiguousarray(v.T).reshape(-1, T.nrow, T.ncol) if name == "frac" else v.reshape(T.nrow, T.ncol)
                assert _bits(v, want[name]) and _bits(v, dp[name].cpu().numpy()), (T, layer, name)
            assert [info[0]] + list(info[2:]) == [float(winfo[k]) for k in ("K", "n_valid", "n_na", "n_other")] and list(codes) == winfo["codes"] == dinfo["codes"]
    T = targets[0]
    out = R.values(R.call("mhsr_class_aggregate", R.geom(S), R.num(z[0]), R.num([np.nan]), R.geom(T), R.num([0]), R.int(CODES), R.NULL, R.int([1 | 4])))
    planes = R.values(out[0])
    want, _ = cr.aggregate(z[0], S, T, CODES)
    assert all(planes[k] == R.NULL for k in (1, 3, 4, 5)) and _bits(R.values(planes[0]).reshape(15, 26), want["mode"]) and _bits(R.values(planes[2]).reshape(15, 26), want["n"])
    args = lambda opts=(0,), pm=1, cl=CODES, fo=None, gd=T, pl=None: (R.geom(S), pl if pl is not None else R.mat(values), R.num([np.nan]), R.geom(gd),  # noqa: E731
                                                                     R.num(list(opts)), R.int(cl) if cl is not None else R.NULL,
                                                                     R.int(fo) if fo is not None else R.NULL, R.int([pm]))
    with pytest.raises(RuntimeError, match="products must be"):
        R.call("mhsr_class_aggregate", *args(pm=0))
    with pytest.raises(RuntimeError, match="products must be"):
        R.call("mhsr_class_aggregate", *args(pm=64))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_class_aggregate", *args(opts=(0, 1)))
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_class_aggregate", *args(opts=(2,)))
    with pytest.raises(RuntimeError, match="twice"):
        R.call("mhsr_class_aggregate", *args(cl=[1, 1]))
    with pytest.raises(RuntimeError, match="is not one of the 5 classes"):
        R.call("mhsr_class_aggregate", *args(pm=32, fo=[12]))
    with pytest.raises(RuntimeError, match="cell size must be finite and positive"):
        R.call("mhsr_class_aggregate", *args(gd=Geometry(1000.0, 5000.0, 0.0, 90.0, 15, 26)))
    with pytest.raises(RuntimeError, match="bad target dimension"):
        R.call("mhsr_class_aggregate", *args(gd=Geometry(1000.0, 5000.0, 90.0, 90.0, 0, 26)))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_class_aggregate", *args(pl=R.mat(values[:-1])))
