"""GPU: flow paths along the D8 forest (include/machisplin_hip.h, section "flow paths"; csrc/flowpath.hip).  All five products --
index, steps, dist, value, drop -- and every count of the info equal the numpy restatement of tests/flowpath_ref.py BIT FOR BIT: no
tolerance appears anywhere, NaN matches NaN.

Planes: the direction planes that tests/hydro_ref.py makes of its noise, tilted, bowl, constant, holes and all-NA surfaces at
the degenerate shapes, one past a 32 x 64 tile in both directions and several tiles, its 96 x 96 spiral, and two hand-made
serpentines whose single path of 2 144 and 9 099 steps crosses every tile border and needs 12 and 14 global rounds -- the
smallest inputs that run many rounds and end on either buffer of the ping-pong.  Each plane is crossed with the targets (none,
every cell, flowacc >= 1 / 20 / 1e9), with and without the root as a target, with and without the local phase."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flowpath_ref as fr
import hydro_ref as hr
import proximity_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DX, DY = 30.0, 20.0
ALL = ("index", "steps", "dist", "value", "drop")
INFO = ("n_valid", "n_targets", "n_roots", "n_unreached", "max_steps")
E, SE, S, SW, W, NW, N, NE, OUT, NA = 0, 1, 2, 3, 4, 5, 6, 7, -1, -2


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "flowpath_rule.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


TH, TW = _constant("FLOW_TH"), _constant("FLOW_TW")
SHAPES = ((1, 1), (1, 70), (70, 1), (2, 2), (TH + 1, TW + 1), (3 * TH + 1, 2 * TW + 2))
PLANES = [(k, s) for k in hr.KINDS for s in SHAPES] + [("spiral", (96, 96)), ("serpentine", (TH + 1, TW + 1)), ("serpentine", (70, 130))]
TARGETS = (("outlet", None), ("valid", None), ("ge", 1.0), ("ge", 20.0), ("ge", 1e9))


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def _plane(kind, shape):
    """(flowdir int8, layers: the accumulation and the heights, float64 with NaN at NA)"""
    if kind == "serpentine":
        d = fr.serpentine(*shape)
        end, ew, ns, dg = fr.walk(d, np.zeros(shape, bool))
        acc = (shape[0] * shape[1] - (ew + ns + dg)).astype(np.float64)              # the cells upstream of a cell, itself included
        return d, np.stack([acc, np.floor(acc / 7.0)])
    z, d, acc = fr.hydro_plane(kind, shape, DX, DY)
    return d, np.stack([acc, z])


def _stack(hip, layers, nodata=NAN, pad=0):
    """a RasterStack of cells of DX x DY; pad > 0: cut out of a tensor with `pad` more columns and one more layer"""
    import torch
    layers = np.asarray(layers)
    n, nr, nc = layers.shape
    geom = hip.Geometry(1000.0, 5000.0, DX, DY, nr, nc)
    st = hip.RasterStack(geom, layers, nodata)
    if pad:
        big = torch.full((n + 1, nr, nc + pad), 5, dtype=st.planes.dtype, device=st.planes.device)
        big[1:, :, :nc] = st.planes
        st.planes = big[1:, :, :nc]
        assert st.planes.stride(1) == nc + pad
    return st


def _dir(hip, d, pad=0):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(d, dtype=np.int8)).to("cuda")
    if pad:
        big = torch.full((d.shape[0], d.shape[1] + pad), 9, dtype=torch.int8, device=t.device)           # 9: a code that must never be read
        big[:, :d.shape[1]] = t
        t = big[:, :d.shape[1]]
        assert t.stride(0) == d.shape[1] + pad
    return t


def _run(hip, d, stack, **kw):
    kw.setdefault("products", ALL)
    kw.setdefault("value_layer", 1)
    planes, info = hip.flowpath.flowpath(d, stack, **kw)
    return {k: v.cpu().numpy() for k, v in planes.items()}, info


@pytest.mark.parametrize("kind,shape", PLANES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_every_product_and_count_equals_the_restatement(hip, kind, shape):
    d, layers = _plane(kind, shape)
    stack, dev = _stack(hip, layers), _dir(hip, d)
    for where, thr in TARGETS:
        for root in (True, False):
            want, winfo = fr.flowpath(d, layers[0], None, where, thr, root, DX, DY, layers[1])
            for local in (True, False):
                got, info = _run(hip, dev, stack, where=where, threshold=thr, root_is_target=root, local=local)
                what = (kind, shape, where, thr, root, local)
                for k in ALL:
                    assert _same(got[k], want[k]), what + (k,)
                assert {k: info[k] for k in INFO} == {k: winfo[k] for k in INFO}, what
                assert info["rounds"] == winfo["rounds"] if not local else info["rounds"] <= winfo["rounds"], what + (info["rounds"], winfo["rounds"])
                assert info["scratch_bytes"] >= 32 * d.size


def test_serpentines_take_the_rounds_their_length_asks_for(hip):
    for shape, steps, rounds in (((33, 65), 2144, 12), ((70, 130), 9099, 14)):
        d, layers = _plane("serpentine", shape)
        got, info = _run(hip, _dir(hip, d), _stack(hip, layers), local=False)
        assert info["rounds"] == rounds and info["max_steps"] == steps and (got["index"] == got["index"][0, 0]).all()
        got, info = _run(hip, _dir(hip, d), _stack(hip, layers), local=True)
        assert info["rounds"] <= rounds and info["max_steps"] == steps and got["steps"][0, 0] == steps


def test_records_without_counts_for_index_value_and_drop(hip):
    d, layers = _plane("holes", (97, 130))
    stack, dev = _stack(hip, layers), _dir(hip, d)
    want, winfo = fr.flowpath(d, layers[0], None, "ge", 20.0, False, DX, DY, layers[1])
    for local in (True, False):
        got, info = _run(hip, dev, stack, where="ge", threshold=20.0, root_is_target=False, local=local, products=("index", "value", "drop"))
        for k in ("index", "value", "drop"):
            assert _same(got[k], want[k]), (local, k)
        assert info["max_steps"] == -1 and info["n_unreached"] == winfo["n_unreached"] and info["n_targets"] == winfo["n_targets"]
        assert 8 * d.size <= info["scratch_bytes"] < 9 * d.size + 4096
        assert info["rounds"] == winfo["rounds"] if not local else info["rounds"] <= winfo["rounds"]
    one, info = hip.flowpath.flowpath(dev, stack, products="index")                                      # one name: the tensor itself
    assert _same(one.cpu().numpy(), fr.flowpath(d)[0]["index"])


@pytest.mark.parametrize("dtype", ("f64", "f32", "i16"))
def test_plane_types_with_a_nodata_value_and_nan(hip, dtype):
    d, layers = _plane("holes", (33, 65))
    rng = np.random.default_rng(4)
    acc, z = layers[0].copy(), layers[1].copy()
    z[rng.random(z.shape) < 0.1] = NAN                                  # NA values at valid cells: value and drop NaN there
    acc[rng.random(z.shape) < 0.05] = NAN                                # ... and NA cells of the target layer are no targets
    typed = np.stack([hr.as_dtype(acc, dtype), hr.as_dtype(z, dtype)])
    if dtype != "i16":
        typed[1][5, 7] = hr.NODATA                                       # a float plane may hold both
    stack = _stack(hip, typed, hr.NODATA)
    for where, thr in (("ge", 5.0), ("na", None), ("lt", 3.0)):
        want, winfo = fr.flowpath(d, typed[0], hr.NODATA, where, thr, False, DX, DY, typed[1])
        got, info = _run(hip, _dir(hip, d), stack, where=where, threshold=thr, root_is_target=False)
        for k in ALL:
            assert _same(got[k], want[k]), (dtype, where, k)
        assert {k: info[k] for k in INFO} == {k: winfo[k] for k in INFO}


def test_padded_stack_and_padded_direction_plane(hip):
    d, layers = _plane("noise", (97, 130))
    want, _ = fr.flowpath(d, layers[0], None, "ge", 20.0, True, DX, DY, layers[1])
    for local in (True, False):
        got, _ = _run(hip, _dir(hip, d, pad=7), _stack(hip, layers, pad=11), where="ge", threshold=20.0, local=local)
        for k in ALL:
            assert _same(got[k], want[k]), (local, k)


def test_float32_products_are_the_float64_ones_converted_once(hip):
    import torch
    d, layers = _plane("tilted", (97, 130))
    want, _ = fr.flowpath(d, layers[0], None, "ge", 20.0, False, DX, DY, layers[1], f32=True)
    got, _ = _run(hip, _dir(hip, d), _stack(hip, layers), where="ge", threshold=20.0, root_is_target=False, out_dtype=torch.float32)
    for k in ALL:
        assert _same(got[k], want[k]), k
    assert got["dist"].dtype == np.float32 and got["index"].dtype == np.int32


def test_host_entry_and_a_repeated_call_give_the_same_bytes(hip):
    from machisplin_amd import _lib
    d, layers = _plane("holes", (97, 130))
    stack, dev = _stack(hip, layers), _dir(hip, d)
    first, info = _run(hip, dev, stack, where="ge", threshold=20.0, root_is_target=False)
    again, _ = _run(hip, dev, stack, where="ge", threshold=20.0, root_is_target=False)
    for k in ALL:
        assert first[k].tobytes() == again[k].tobytes(), k
    host = {k: np.empty(d.shape, dtype=np.int32 if k in ("index", "steps") else np.float64) for k in ALL}
    out = _lib.FlowpathOut(*[host[k].ctypes.data for k in ALL])
    hinfo = _lib.FlowpathInfo()
    g = stack.geom.c_struct()
    pad = np.full((d.shape[0], d.shape[1] + 3), 9, dtype=np.int8)
    pad[:, :d.shape[1]] = d
    cs = _lib.Stack(layers.ctypes.data, 2, _lib.F64, d.size, d.shape[1], NAN)
    _lib.check(_lib.lib().mhs_flowpath(C.byref(g), pad.ctypes.data, pad.shape[1], C.byref(cs), 0, 5, 20.0, 1, 0, DX, DY, C.byref(out), _lib.F64,
                                       C.byref(hinfo)))
    for k in ALL:
        assert first[k].tobytes() == host[k].tobytes(), k
    assert {k: getattr(hinfo, k) for k in INFO + ("rounds",)} == {k: info[k] for k in INFO + ("rounds",)}


def test_malformed_planes_and_cycles_are_refused_and_the_library_stays_usable(hip):
    d, layers = _plane("noise", (33, 65))
    stack = _stack(hip, layers)
    want, _ = fr.flowpath(d, layers[0], None, "ge", 20.0, True, DX, DY, layers[1])

    def good():
        got, _ = _run(hip, _dir(hip, d), stack, where="ge", threshold=20.0)
        assert all(_same(got[k], want[k]) for k in ALL)

    for code, at in ((8, (5, 5)), (-3, (32, 64)), (127, (0, 0)), (W, (7, 0)), (S, (32, 9))):       # a bad code; out of the raster west and south
        bad = d.copy()
        bad[at] = code
        for local in (True, False):
            with pytest.raises(hip.MhsError, match="flowdir is malformed") as ei:
                _run(hip, _dir(hip, bad), stack, local=local)
            assert ei.value.code == hip._lib.ERR_INVALID
        good()
    holes, hl = _plane("holes", (33, 65))
    r, c = (int(x[0]) for x in np.nonzero(holes == NA))
    bad = holes.copy()
    bad[r, c - 1] = E                                                                               # points at an NA cell
    with pytest.raises(hip.MhsError, match="flowdir is malformed"):
        _run(hip, _dir(hip, bad), _stack(hip, hl))
    good()
    two = _stack(hip, np.zeros((2, 1, 2)))
    three = _stack(hip, np.zeros((2, 2, 2)))
    for local in (True, False):
        with pytest.raises(hip.MhsError, match="flowdir has a cycle") as ei:                        # 2 cells: would fold into self-pointers
            _run(hip, _dir(hip, np.array([[E, W]])), two, local=local)
        assert ei.value.code == hip._lib.ERR_INVALID
        with pytest.raises(hip.MhsError, match="flowdir has a cycle"):                              # 3 cells: never settles, the round bound ends it
            _run(hip, _dir(hip, np.array([[E, SW], [N, W]])), three, local=local)
    cyc = fr.serpentine(40, 70)
    cyc[39, 69], cyc[38, 69] = N, W                                                                 # 2 700 cells run into a cycle of 2
    with pytest.raises(hip.MhsError, match="flowdir has a cycle"):
        _run(hip, _dir(hip, cyc), _stack(hip, np.zeros((2, 40, 70))))
    good()


def _two_valleys():
    """60 x 40, tilted to the south: a valley floor in column 5 and one, 55 higher, in column 30, the ridge between them in
    column 26 -- so columns 20 .. 24 drain WEST into the far valley while the near one, across the ridge, is the nearest as the
    crow flies"""
    r, c = np.meshgrid(np.arange(60.0), np.arange(40.0), indexing="ij")
    return np.where(c <= 25, 10.0 * np.abs(c - 5), 55.0 + 40.0 * np.abs(c - 30)) + 3.0 * (60 - r)


def test_covariates_along_the_flow(hip):
    import torch
    from machisplin_amd import terrain
    z = hr.plane("holes", (97, 130))
    geom = hip.Geometry(1000.0, 5000.0, DX, DY, 97, 130)
    st = hip.RasterStack(geom, z[None], NAN)
    cov = terrain.covariates(st, (("hand", 20), "twi", ("flowdist_stream", 20), "flowdist_outlet", ("hand", 5), "slope_deg"))
    assert cov.names == ["dem", "hand20", "twi", "flowdist_stream20", "flowdist_outlet", "hand5", "slope_deg"] and cov.planes.dtype == torch.float32
    _, d, acc = fr.hydro_plane("holes", (97, 130), DX, DY)
    got = cov.planes.cpu().numpy()
    for a, k_hand, k_dist in ((20.0, 1, 3), (5.0, 5, None)):
        want, _ = fr.flowpath(d, acc, None, "ge", a, True, DX, DY, z, f32=True)
        assert _same(got[k_hand], want["drop"]), a
        if k_dist:
            assert _same(got[k_dist], want["dist"]), a
    assert _same(got[4], fr.flowpath(d, dx=DX, dy=DY, f32=True)[0]["dist"])
    hp, _ = terrain.hydro(st, 0, "twi")
    assert torch.equal(cov.planes[2].view(torch.int32), hp.to(torch.float32).view(torch.int32))                  # the shared hydro call
    assert torch.equal(cov.planes[6].view(torch.int32), terrain.terrain(st, 0, ("slope_deg",), out_dtype=torch.float32)[0].view(torch.int32))
    for spec in ((("hand", 20),), ("flowdist_outlet",), (("flowdist_stream", 3), "twi")):
        with pytest.raises(ValueError, match="lonlat"):
            terrain.covariates(st, spec, lonlat=True)
    with pytest.raises(ValueError, match="hand"):
        terrain.covariates(st, ("hand",))
    with pytest.raises(ValueError, match="flowdist_outlet"):
        terrain.covariates(st, (("flowdist_outlet", 3),))


def test_hand_follows_the_water_where_above_stream_crosses_the_ridge(hip):
    from machisplin_amd import terrain
    z = _two_valleys()
    st = hip.RasterStack(hip.Geometry(0.0, 1800.0, 30.0, 30.0, 60, 40), z[None], NAN)
    cov = terrain.covariates(st, (("hand", 30), ("above_stream", 30)))
    hand, above = cov.planes[1].cpu().numpy(), cov.planes[2].cpu().numpy()
    h = hr.hydro(z, NAN, 30.0, 30.0)
    want, _ = fr.flowpath(h["flowdir"], h["flowacc"], None, "ge", 30.0, True, 30.0, 30.0, z, f32=True)
    assert _same(hand, want["drop"])
    idx = want["index"][10:50, 20:25]
    assert (idx % 40 == 5).all()                                                                     # the water of these cells reaches the west valley
    near = pr.proximity(h["flowacc"], None, "ge", 30.0)["index"][10:50, 20:25]
    assert (near % 40 == 30).all()                                                                   # ... but the east one is nearer
    assert (hand[10:50, 20:25] != above[10:50, 20:25]).all() and (hand[10:50, 20:25] >= 150).all()
    assert (hand[h["flowacc"] >= 30] == 0).all()


def test_a_spec_without_the_new_names_is_what_the_existing_functions_compose(hip):
    import torch
    from machisplin_amd import terrain
    z = hr.plane("holes", (97, 130))
    st = hip.RasterStack(hip.Geometry(1000.0, 5000.0, 30.0, 30.0, 97, 130), z[None], NAN)
    cov = terrain.covariates(st, ("slope_deg", ("dist_stream", 20), "twi", ("above_stream", 20), "log_flowacc", "dist_na", ("above_min", 3)))
    assert cov.names == ["dem", "slope_deg", "dist_stream20", "twi", "above_stream20", "log_flowacc", "dist_na", "above_min3"]
    hp, _ = terrain.hydro(st, 0, ("twi", "flowacc"))
    dem64 = st.planes[0].to(torch.float64)
    pair = hip.RasterStack(st.geom, torch.stack([hp["flowacc"], dem64]), NAN)
    sp, _ = hip.proximity.proximity(pair, 0, "ge", 20.0, ("dist", "value"), value_layer=1)
    parts = [st.planes[0].to(torch.float32), terrain.terrain(st, 0, ("slope_deg",), out_dtype=torch.float32)[0], sp["dist"].to(torch.float32),
             hp["twi"].to(torch.float32), (dem64 - sp["value"]).to(torch.float32), torch.log(hp["flowacc"]).to(torch.float32),
             hip.proximity.proximity(st, 0, "na", None, "dist", out_dtype=torch.float32)[0], terrain.relief(st, 3, "above_min", out_dtype=torch.float32)]
    for k, p in enumerate(parts):
        assert torch.equal(cov.planes[k].view(torch.int32), p.reshape(97, 130).view(torch.int32)), cov.names[k]
