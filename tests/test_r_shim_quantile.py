"""GPU: the quantile entry of the R .Call() shim (mhsr_zonal_quantile -> the host entry point mhs_zonal_quantile on double planes
with the layout of terra::values), executed through the stand-in R runtime, equals the restatement (tests/quantile_ref.py) bit
for bit: a zone plane in the present and the dense form, the whole layer, and a target grid.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import quantile_ref as qr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
PROBS = (0.5, 0.0, 0.9, 1.0)


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_shim_quantile_equals_the_restatement_exactly(R, hip):  # noqa: F811
    from machisplin_amd import Geometry
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)
    rng = np.random.default_rng(12)
    z = np.stack([rng.integers(0, 6000, (45, 77)) / 8.0, np.round(rng.standard_normal((45, 77)), 2)])
    z[0, rng.integers(0, 45, 300), rng.integers(0, 77, 300)] = np.nan
    z[0, 20:24, 30:37] = -9999.0
    zones = rng.integers(0, 30, (45, 77)).astype(np.int32)
    zones[zones == 7] = 300
    zones[rng.random((45, 77)) < 0.05] = NA_INTEGER
    values = z.reshape(2, -1).T
    for layer, nz in ((0, 301), (1, 0)):
        want = qr.quantile(z[layer], zones, PROBS, -9999.0, n_zones=nz or None)
        for present in (1, 0):
            out = R.values(R.call("mhsr_zonal_quantile", R.geom(g), R.mat(values), R.num([-9999.0]), R.int(zones), R.NULL,
                                  R.num([layer, nz, 0.0, present, 1, 7]), R.num(PROBS)))
            tab, planes, info = R.values(out[0]), R.values(out[1]), R.values(out[2])
            wt = qr.present(want[0]) if present else want[0]
            if present:
                assert _bits(R.values(tab[0]), wt["zone"])
            else:
                assert tab[0] == R.NULL
            assert _bits(R.values(tab[1]), wt["count"].astype(np.float64))
            assert _bits(R.values(tab[2]).reshape(-1, len(PROBS)), wt["q"])
            qp = R.values(planes[0])
            for j in range(len(PROBS)):
                assert _bits(R.values(qp[j]).reshape(45, 77), want[1]["q"][j]), (layer, present, j)
            assert _bits(R.values(planes[1]).reshape(45, 77), want[1]["below"]) and _bits(R.values(planes[2]).reshape(45, 77), want[1]["frac_below"])
            assert list(info)[:7] == [float(want[2][k]) for k in qr.INFO] and 0 <= info[7] <= 8
    # the whole layer: a table only
    want = qr.quantile(z[1], None, PROBS)
    out = R.values(R.call("mhsr_zonal_quantile", R.geom(g), R.num(z[1]), R.num([np.nan]), R.NULL, R.NULL, R.num([0, 0, 0, 0, 1, 0]), R.num(PROBS)))
    tab, planes = R.values(out[0]), R.values(out[1])
    assert _bits(R.values(tab[2]).reshape(1, -1), want[0]["q"]) and planes[0] == R.NULL and planes[1] == R.NULL and planes[2] == R.NULL
    # a target grid
    T = Geometry(1040.0, 4980.0, 111.0, 140.0, 11, 21)
    wq, wc, _ = qr.aggregate_quantile(z[0], g, T, PROBS, -9999.0)
    out = R.values(R.call("mhsr_zonal_quantile", R.geom(g), R.mat(values), R.num([-9999.0]), R.NULL, R.geom(T), R.num([0, 0, 0, 0, 1, 0]), R.num(PROBS)))
    tab = R.values(out[0])
    assert _bits(R.values(tab[2]).reshape(-1, len(PROBS)).T.reshape(wq.shape).copy(), wq) and _bits(R.values(tab[1]).reshape(wc.shape), wc.astype(np.float64))
    assert (wc == 0).any()
    # refusals come back as R errors
    args = lambda opts, zz=R.int(zones), tg=R.NULL, pr=R.num(PROBS): (R.geom(g), R.mat(values), R.num([-9999.0]), zz, tg, R.num(opts), pr)   # noqa: E731
    for bad in (args([0, 300, 0, 0, 1, 0]), args([0, 0, 3.0, 0, 1, 0]), args([0, 0, 0, 0, 0, 0]), args([0, 0, 0, 0, 1, 0], tg=R.geom(T)),
                args([0, 0, 0, 0, 1, 0], pr=R.num([0.5, 1.5])), args([0, 5, 0, 0, 1, 0], zz=R.NULL), args([0, 0, 0, 0, 1, 8])):
        with pytest.raises(Exception):
            R.call("mhsr_zonal_quantile", *bad)
