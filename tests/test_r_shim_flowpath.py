"""GPU: the flow-path entry of the R .Call() shim (mhsr_flowpath -> the host entry point mhs_flowpath on double planes with the
layout of terra::values and the integer direction vector mhsr_hydro returns), executed through the stand-in R runtime of
tests/rstub, equals the Python call on device planes and the restatement (tests/flowpath_ref.py) bit for bit.  Bad arguments
come back as R errors."""
import numpy as np
import pytest

import flowpath_ref as fr
import hydro_ref as hr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31
ALL = ("index", "steps", "dist", "value", "drop")
INFO = ("n_valid", "n_targets", "n_roots", "n_unreached", "max_steps", "rounds")


def test_shim_flowpath_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    import torch
    from machisplin_amd import Geometry
    from machisplin_amd.flowpath import flowpath
    R.call("mhsr_init", R.int([0]))
    g = Geometry(1000.0, 5000.0, 30.0, 20.0, 45, 77)
    z, d, acc = fr.hydro_plane("holes", (45, 77), 30.0, 20.0)
    rng = np.random.default_rng(12)
    v = np.where(rng.random(z.shape) < 0.1, -9999.0, z)                                  # a nodata value at valid cells of the value layer
    layers = np.stack([acc, v])
    stack = hip.RasterStack(g, layers, -9999.0)
    dev = torch.from_numpy(d).to("cuda")
    values = layers.reshape(2, -1).T                                                     # terra::values: ncell x C
    rdir = np.where(d == hr.DIR_NA, NA_INTEGER, d.astype(np.int64)).ravel()              # as mhsr_hydro hands the directions over
    for code, where, thr, root in ((8, "outlet", None, True), (5, "ge", 20.0, True), (5, "ge", 20.0, False), (0, "na", None, False),
                                   (2, "lt", 3.0, True)):
        want, want_info = flowpath(dev, stack, 0, where, thr, ALL, value_layer=1, root_is_target=root)
        want = {k: p.cpu().numpy() for k, p in want.items()}
        ref, _ = fr.flowpath(d, acc, -9999.0, where, thr, root, 30.0, 20.0, v)
        out = R.values(R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([-9999.0]),
                              R.num([0, code, thr or 0.0, 1, 1 if root else 0, 30.0, 20.0]), R.int([31])))
        assert len(out) == 6
        for k, name in enumerate(ALL):
            p = R.values(out[k]).reshape(45, 77)
            if name in ("index", "steps"):
                p = np.where(p == NA_INTEGER, -1, p - 1 if name == "index" else p).astype(np.int32)      # a terra cell number; NA_integer_
            assert p.dtype == want[name].dtype and np.array_equal(p, want[name], equal_nan=True), (where, name)
            assert np.array_equal(p, ref[name], equal_nan=True), (where, name)
        assert list(R.values(out[5])) == [want_info[k] for k in INFO]
    # a subset: the planes not asked for are NULL; one layer as a plain vector; value_layer and the units are not looked at
    out = R.values(R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.num(acc), R.num([np.nan]), R.num([0, 8, 0.0, -1, 2, 0.0, 0.0]), R.int([1])))
    assert all(out[k] == R.NULL for k in (1, 2, 3, 4))
    labels = R.values(out[0]).reshape(45, 77)
    assert np.array_equal(np.where(labels == NA_INTEGER, -1, labels - 1), fr.flowpath(d)[0]["index"])
    assert list(R.values(out[5]))[4] == -1.0                                              # max_steps: the counts were not carried
    # refusals of the library and of the shim come back as R errors
    bad = rdir.copy(); bad[100] = 9
    with pytest.raises(RuntimeError, match="flowdir is malformed"):
        R.call("mhsr_flowpath", R.geom(g), R.int(bad), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([31]))
    g2 = Geometry(0.0, 1.0, 1.0, 1.0, 1, 2)
    with pytest.raises(RuntimeError, match="flowdir has a cycle"):
        R.call("mhsr_flowpath", R.geom(g2), R.int([0, 4]), R.num(np.zeros(2)), R.num([np.nan]), R.num([0, 8, 0.0, -1, 1, 1.0, 1.0]), R.int([3]))
    with pytest.raises(RuntimeError, match="dx and dy"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 0.0, 20.0]), R.int([4]))
    with pytest.raises(RuntimeError, match="value_layer"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 2, 1, 30.0, 20.0]), R.int([16]))
    with pytest.raises(RuntimeError, match="layer"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([2, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([1]))
    with pytest.raises(RuntimeError, match="bit mask"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([32]))
    with pytest.raises(RuntimeError, match="where must be"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 9, 0.0, 1, 1, 30.0, 20.0]), R.int([1]))
    with pytest.raises(RuntimeError, match="flags must be"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 4, 30.0, 20.0]), R.int([1]))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1]), R.int([1]))
    with pytest.raises(RuntimeError, match="one code per cell"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir[:-1]), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([1]))
    with pytest.raises(RuntimeError, match="one code per cell"):
        R.call("mhsr_flowpath", R.geom(g), R.num(rdir), R.mat(values), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([1]))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_flowpath", R.geom(g), R.int(rdir), R.mat(values[:-1]), R.num([np.nan]), R.num([0, 8, 0.0, 1, 1, 30.0, 20.0]), R.int([1]))
