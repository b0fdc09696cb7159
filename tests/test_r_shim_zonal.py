"""GPU: the zonal entry of the R .Call() shim (mhsr_zonal -> the host entry point mhs_zonal on double planes with the layout of
terra::values), executed through the stand-in R runtime of tests/rstub, equals the Python call on device planes and the
restatement (tests/zonal_ref.py) bit for bit.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import zonal_ref as zr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
ALL, TAB = zr.STATS, zr.TABLE_STATS
ALL_BITS, TAB_BITS = 4095, 0x87f


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_shim_zonal_equals_the_device_call_exactly(R, hip):  # noqa: F811
    import torch
    from machisplin_amd import Geometry
    from machisplin_amd.zonal import zonal
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)                                   # two tiles side by side, two above each other
    rng = np.random.default_rng(12)
    z = np.stack([rng.integers(0, 6000, (45, 77)) / 8.0, np.round(rng.standard_normal((45, 77)), 2)])
    z[0, rng.integers(0, 45, 300), rng.integers(0, 77, 300)] = np.nan                  # NA_real_ cells
    z[0, 20:24, 30:37] = -9999.0                                                       # ... and a nodata value
    zones = rng.integers(0, 30, (45, 77)).astype(np.int32)
    zones[:, 40:60] = 11
    zones[zones == 7] = 300                                                            # a gap in the numbering: the present form skips it
    zones[rng.random((45, 77)) < 0.05] = NA_INTEGER                                    # NA_integer_: no zone
    zones[3, 3] = -5
    stack = hip.RasterStack(g, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    for layer, nz, quantum in ((0, 301, 0.0), (1, 0, 0.0), (0, 400, 2.0 ** -10)):
        want = zr.zonal(z[layer], zones, -9999.0, n_zones=nz or None, quantum=quantum or None)
        dt, dp, dinfo = zonal(stack, torch.from_numpy(zones), layer, TAB, ALL, nz or None, "present", quantum or None)
        for present in (1, 0):
            out = R.values(R.call("mhsr_zonal", R.geom(g), R.mat(values), R.num([-9999.0]), R.int(zones), R.num([layer, nz, quantum, present]),
                                  R.int([TAB_BITS]), R.int([ALL_BITS])))
            assert len(out) == 3
            tab, planes, info = R.values(out[0]), R.values(out[1]), R.values(out[2])
            assert len(tab) == 9 and len(planes) == 12
            wt = zr.present(want[0]) if present else want[0]
            if present:
                assert _bits(R.values(tab[0]), wt["zone"]) and _bits(R.values(tab[0]), dt["zone"].cpu().numpy())
            else:
                assert tab[0] == R.NULL
            for k, name in enumerate(TAB):
                v = R.values(tab[1 + k])
                assert v.dtype == np.float64 and _bits(v, wt[name].astype(np.float64)), (layer, present, name)
                if present:
                    assert _bits(v, dt[name].cpu().numpy().astype(np.float64)), name
            for k, name in enumerate(ALL):
                v = R.values(planes[k]).reshape(45, 77)
                assert _bits(v, want[1][name]) and _bits(v, dp[name].cpu().numpy()), (layer, present, name)
            assert list(info) == [float(want[2][k]) for k in zr.INFO] and list(info) == [float(dinfo[k]) for k in zr.INFO]
    # a subset: what is not asked for is NULL; one layer as a plain vector; planes only; a table only
    want = zr.zonal(z[1], zones)
    out = R.values(R.call("mhsr_zonal", R.geom(g), R.num(z[1]), R.num([np.nan]), R.int(zones), R.num([0, 0, 0, 0]), R.int([4 | 2048]), R.int([128])))
    tab, planes = R.values(out[0]), R.values(out[1])
    assert all(tab[k] == R.NULL for k in (0, 1, 2, 4, 5, 6, 7)) and all(planes[k] == R.NULL for k in range(12) if k != 7)
    assert _bits(R.values(tab[3]), want[0]["mean"]) and _bits(R.values(tab[8]), want[0]["cells"].astype(np.float64))
    assert _bits(R.values(planes[7]).reshape(45, 77), want[1]["minus_mean"])
    out = R.values(R.call("mhsr_zonal", R.geom(g), R.num(z[1]), R.num([np.nan]), R.int(zones), R.num([0, 0, 0, 1]), R.int([0]), R.int([1024])))
    assert all(t == R.NULL for t in R.values(out[0])) and _bits(R.values(R.values(out[1])[10]).reshape(45, 77), want[1]["dev"])
    # no zone anywhere: an empty table, NaN planes, and the call succeeds
    nowhere = np.full((45, 77), NA_INTEGER, dtype=np.int32)
    for present in (0, 1):
        out = R.values(R.call("mhsr_zonal", R.geom(g), R.num(z[1]), R.num([np.nan]), R.int(nowhere), R.num([0, 0, 0, present]), R.int([4]), R.int([4 | 1])))
        assert R.values(R.values(out[0])[3]).size == 0 and np.isnan(R.values(R.values(out[1])[2])).all() and (R.values(R.values(out[1])[0]) == 0).all()
        assert list(R.values(out[2]))[:4] == [0.0, 0.0, 0.0, 0.0]
    # refusals of the library and of the shim come back as R errors
    args = lambda opts, ts=4, ps=0, zn=zones, pl=None: (R.geom(g), pl if pl is not None else R.mat(values), R.num([np.nan]), R.int(zn), R.num(opts),  # noqa: E731
                                                        R.int([ts]), R.int([ps]))
    with pytest.raises(RuntimeError, match="n_zones"):
        R.call("mhsr_zonal", *args([0, 300, 0, 0]))                                    # zone 300 is not below 300
    with pytest.raises(RuntimeError, match="quantum"):
        R.call("mhsr_zonal", *args([0, 0, 3.0, 0]))
    with pytest.raises(RuntimeError, match="quantum"):
        R.call("mhsr_zonal", *args([0, 0, 2.0 ** -40, 1]))                             # too small for values of several hundred
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_zonal", *args([2, 0, 0, 0]))
    with pytest.raises(RuntimeError, match="no output"):
        R.call("mhsr_zonal", *args([0, 0, 0, 0], ts=0))
    with pytest.raises(RuntimeError, match="stats must be"):
        R.call("mhsr_zonal", *args([0, 0, 0, 0], ts=128))
    with pytest.raises(RuntimeError, match="planes_mask must be"):
        R.call("mhsr_zonal", *args([0, 0, 0, 0], ps=4096))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_zonal", *args([0, 0, 0]))
    with pytest.raises(RuntimeError, match="one zone per cell"):
        R.call("mhsr_zonal", *args([0, 0, 0, 0], zn=zones[:-1]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_zonal", *args([0, 0, 0, 0], pl=R.mat(values[:-1])))
