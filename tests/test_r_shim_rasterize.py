"""GPU: the rasterize entry of the R .Call() shim (mhsr_rasterize -> the host entry point mhs_rasterize, with R's column-major
coordinate matrix and integer offsets), executed through the stand-in R runtime of tests/rstub, equals the Python call on device
planes and the restatement (tests/rasterize_ref.py) bit for bit.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import rasterize_ref as rr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

KINDS = ("point", "line", "polygon")


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _args(R, g, ft, rule="last", touches=False, budget=0, products=7, values="default", opts=None, coords=None, parts=None, feats=None):  # noqa: F811
    vals = (R.NULL if ft.values is None else R.num(ft.values)) if isinstance(values, str) else values
    return (R.geom(g), R.mat(ft.coords) if coords is None else coords, R.int(ft.part_offsets) if parts is None else parts,
            R.int(ft.feature_offsets) if feats is None else feats, vals,
            R.num([KINDS.index(ft.kind), rr.RULES.index(rule), float(touches), budget] if opts is None else opts), R.int([products]))


def test_shim_rasterize_equals_the_device_call_exactly(R, hip):  # noqa: F811
    from machisplin_amd import Geometry
    from machisplin_amd.rasterize import rasterize
    from machisplin_amd.vector import Features
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 45, 77)
    rng = np.random.default_rng(12)
    units = Features.from_parts("polygon", [[r] for r in rr.lattice(g, 3, 4, 1, zigzag=2)][1:] +
                                [[rr.star(2200.0, 4300.0, 200.0, 500.0, 15, 3), rr.star(2200.0, 4300.0, 50.0, 150.0, 6, 4)]], rng.integers(0, 4, 12).astype(float))
    rivers = Features.from_parts("line", [[np.column_stack([rng.uniform(900.0, 3400.0, 8), rng.uniform(3600.0, 5100.0, 8)])] for _ in range(3)], [3.0, 1.0, 2.0])
    pts = np.column_stack([rng.uniform(900.0, 3400.0, 500), rng.uniform(3600.0, 5100.0, 500)])
    stations = Features("point", pts, np.arange(501), np.arange(501), rng.integers(0, 9, 500).astype(float))
    for ft, rule, touches, budget in ((units, "last", False, 0), (units, "max", True, 0), (units, "min", True, 300), (rivers, "first", False, 0),
                                      (stations, "max", False, 0)):
        want, winfo = rr.rasterize(ft, g, rule, touches)
        dev, dinfo = rasterize(ft, g, ("index", "count", "value"), rule, touches, scratch_budget=budget or None)
        out = R.values(R.call("mhsr_rasterize", *_args(R, g, ft, rule, touches, budget)))
        assert len(out) == 4
        for k, name in enumerate(("index", "count", "value")):
            v = R.values(out[k]).reshape(45, 77)
            assert _bits(v, want[name]) and _bits(v, dev[name].cpu().numpy()), (ft.kind, rule, name)
        info = R.values(out[3])
        names = ("n_features", "n_parts", "n_vertices", "n_edges", "n_items", "n_batches", "n_burned", "n_outside")
        assert list(info) == [float(dinfo[k]) for k in names]
        assert all(info[names.index(k)] == winfo[k] for k in rr.INFO)
        if budget:
            assert info[5] > 1
    # a subset: what is not asked for is NULL; no values where none are needed
    plain = Features(units.kind, units.coords, units.part_offsets, units.feature_offsets)
    out = R.values(R.call("mhsr_rasterize", *_args(R, g, plain, products=2)))
    assert out[0] == R.NULL and out[2] == R.NULL and _bits(R.values(out[1]).reshape(45, 77), rr.rasterize(plain, g)[0]["count"])
    # no feature at all: nothing burned, and the call succeeds
    none = Features("polygon", np.zeros((0, 2)), [0], [0])
    out = R.values(R.call("mhsr_rasterize", *_args(R, g, none, products=3)))
    assert (R.values(out[0]) == -1).all() and (R.values(out[1]) == 0).all() and list(R.values(out[3])) == [0.0] * 5 + [1.0, 0.0, 0.0]
    # refusals of the library and of the shim come back as R errors
    with pytest.raises(RuntimeError, match="values is missing"):
        R.call("mhsr_rasterize", *_args(R, g, plain, products=4))
    with pytest.raises(RuntimeError, match="values is missing"):
        R.call("mhsr_rasterize", *_args(R, g, plain, rule="max", products=1))
    open_ring = units.coords.copy()
    open_ring[0, 0] += 1.0
    with pytest.raises(RuntimeError, match="ring 0 is not closed"):
        R.call("mhsr_rasterize", *_args(R, g, units, coords=R.mat(open_ring)))
    open_ring[0, 0] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        R.call("mhsr_rasterize", *_args(R, g, units, coords=R.mat(open_ring)))
    with pytest.raises(RuntimeError, match="part_offsets must start at 0 and end at n_vertices"):
        R.call("mhsr_rasterize", *_args(R, g, units, parts=R.int(units.part_offsets[:-1]), feats=R.int(units.feature_offsets - np.r_[0, np.ones(12, int)])))
    with pytest.raises(RuntimeError, match="feature_offsets must not decrease"):
        R.call("mhsr_rasterize", *_args(R, g, units, feats=R.int(np.r_[units.feature_offsets[:3], 1, units.feature_offsets[4:]])))
    with pytest.raises(RuntimeError, match="two columns"):
        R.call("mhsr_rasterize", *_args(R, g, units, coords=R.num(units.coords.ravel())))
    with pytest.raises(RuntimeError, match="one value per feature"):
        R.call("mhsr_rasterize", *_args(R, g, units, values=R.num([1.0, 2.0])))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_rasterize", *_args(R, g, units, opts=[2, 0, 0]))
    with pytest.raises(RuntimeError, match="kind must be"):
        R.call("mhsr_rasterize", *_args(R, g, units, opts=[3, 0, 0, 0]))
    with pytest.raises(RuntimeError, match="rule must be"):
        R.call("mhsr_rasterize", *_args(R, g, units, opts=[2, 4, 0, 0]))
    with pytest.raises(RuntimeError, match="scratch_budget"):
        R.call("mhsr_rasterize", *_args(R, g, units, opts=[2, 0, 0, -1]))
    with pytest.raises(RuntimeError, match="products must be"):
        R.call("mhsr_rasterize", *_args(R, g, units, products=0))
    with pytest.raises(RuntimeError, match="products must be"):
        R.call("mhsr_rasterize", *_args(R, g, units, products=8))
    with pytest.raises(RuntimeError, match="integer vector"):
        R.call("mhsr_rasterize", *_args(R, g, units, parts=R.num(units.part_offsets)))
