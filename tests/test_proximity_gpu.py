"""GPU: exact Euclidean proximity (include/machisplin_hip.h, section "proximity"; csrc/proximity.hip).  All six products --
d2, index, dist, dir_x, dir_y, value -- equal the two-stage numpy restatement of tests/proximity_ref.py BIT FOR BIT: no
tolerance appears anywhere, NaN matches NaN.

Shapes: the degenerate ones, sizes that are no multiple of a wave, and one past each size at which the kernels change path --
PROX_CHUNK (the columns a wave scans at once), PROX_PRELOAD (the rows a lane loads ahead), PROX_BAND (the rows a lane walks
from one binary search) and PROX_TOP (the stack entries a lane keeps in LDS), read from the text of csrc/proximity_rule.h.  Each shape is crossed with the masks that stress the tie
rule and the envelope: single corners, nothing, everything, full and last rows and columns, a diagonal, a checkerboard, mirrored
pairs, random masks at three densities.  1 x 46 000 and 46 000 x 1 with the one feature at the end reach d2 = 2 115 908 001,
just under the int32 limit: the smallest input that exposes a 32-bit intermediate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import proximity_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
UNIT = 30.0
ALL = ("d2", "index", "dist", "dir_x", "dir_y", "value")


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "proximity_rule.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


CHUNK, PRELOAD, BAND, TOP = _constant("PROX_CHUNK"), _constant("PROX_PRELOAD"), _constant("PROX_BAND"), _constant("PROX_TOP")
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 130), (67, 129), (130, 67), (257, 300), (BAND + 1, CHUNK + 1), (PRELOAD + 1, 2 * CHUNK + 1),
          (4 * BAND + 1, 3), (TOP + 1, 2 * TOP + 3)]


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def masks(nrow, ncol):
    """name -> boolean feature mask"""
    rng = np.random.default_rng(nrow * 1000 + ncol)
    out = {}
    for name, (r, c) in {"corner_nw": (0, 0), "corner_ne": (0, ncol - 1), "corner_sw": (nrow - 1, 0), "corner_se": (nrow - 1, ncol - 1)}.items():
        m = np.zeros((nrow, ncol), bool); m[r, c] = True
        out[name] = m
    out["none"] = np.zeros((nrow, ncol), bool)
    out["all"] = np.ones((nrow, ncol), bool)
    for name, sl in {"row": (nrow // 2, slice(None)), "col": (slice(None), ncol // 2), "last_row": (nrow - 1, slice(None)),
                     "last_col": (slice(None), ncol - 1)}.items():
        m = np.zeros((nrow, ncol), bool); m[sl] = True
        out[name] = m
    # a full column and, further down, a full row: in a column far from the first every row enters the envelope, the full row then
    # pops as many entries as the column is away -- deeper than the PROX_TOP entries kept in LDS -- and the rows below push on
    m = np.zeros((nrow, ncol), bool); m[:, ncol // 2] = True; m[(3 * nrow) // 4, :] = True
    out["col_then_row"] = m
    r, c = np.meshgrid(np.arange(nrow), np.arange(ncol), indexing="ij")
    out["diagonal"] = r == c
    out["checkerboard"] = (r + c) % 2 == 0
    cr, cc, ar, ac = nrow // 2, ncol // 2, min(nrow // 2, 5), min(ncol // 2, 5)
    m = np.zeros((nrow, ncol), bool); m[cr - ar, cc] = m[min(cr + ar, nrow - 1), cc] = True     # mirrored about the ROW cr: ties along it
    out["mirror_row"] = m
    m = np.zeros((nrow, ncol), bool); m[cr, cc - ac] = m[cr, min(cc + ac, ncol - 1)] = True     # mirrored about the cell (cr, cc) in its row
    out["mirror_cell"] = m
    m = np.zeros((nrow, ncol), bool); m[cr - ar, cc - ac] = m[min(cr + ar, nrow - 1), min(cc + ac, ncol - 1)] = True     # ... diagonally
    out["mirror_diag"] = m
    for d in (1e-3, 0.05, 0.5):
        out[f"random{d:g}"] = rng.random((nrow, ncol)) < d
    return out


def _stack(hip, layers, nodata=NAN, pad=0):
    """a RasterStack of square cells of UNIT; pad > 0: cut out of a tensor with `pad` more columns and one more layer"""
    import torch
    layers = np.asarray(layers)
    n, nr, nc = layers.shape
    geom = hip.Geometry(1000.0, 5000.0, UNIT, UNIT, nr, nc)
    st = hip.RasterStack(geom, layers, nodata)
    if pad:
        big = torch.full((n + 1, nr, nc + pad), 5, dtype=st.planes.dtype, device=st.planes.device)
        big[1:, :, :nc] = st.planes
        st.planes = big[1:, :, :nc]
        assert st.planes.stride(1) == nc + pad
    return st


def _run(hip, stack, **kw):
    kw.setdefault("products", ALL)
    planes, info = hip.proximity.proximity(stack, **kw)
    return {k: v.cpu().numpy() for k, v in planes.items()}, info


def _mask_layers(mask, seed=3):
    """layer 0: NaN at the features, 1 elsewhere; layer 1: values with a tenth of the cells NA"""
    rng = np.random.default_rng(seed)
    v = np.round(rng.standard_normal(mask.shape) * 100.0, 1)
    v[rng.random(mask.shape) < 0.1] = np.nan
    return np.stack([np.where(mask, np.nan, 1.0), v])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_product_on_every_mask_equals_the_restatement(hip, shape):
    for name, mask in masks(*shape).items():
        z = _mask_layers(mask)
        got, info = _run(hip, _stack(hip, z), where="na", value_layer=1)
        want = pr.proximity(z[0], None, "na", unit=UNIT, value_plane=z[1])
        for k in ALL:
            assert _same(got[k], want[k]), (shape, name, k)
        assert info["n_features"] == mask.sum() and info["max_d2"] == want["d2"].max(), (shape, name)
        assert info["scratch_bytes"] >= 12 * mask.size + 4 * shape[1]
        if name == "none":
            assert (got["d2"] == -1).all() and (got["index"] == -1).all() and all(np.isnan(got[k]).all() for k in ALL[2:])


def _typed(dtype, nodata):
    """a 67 x 129 plane of the type: small whole values, NA in clusters as the nodata value (and NaN in float planes)"""
    rng = np.random.default_rng(17)
    z = rng.integers(-3, 40, (67, 129)).astype(np.float64)
    z[10:14, 20:90] = nodata if not np.isnan(nodata) else np.nan
    z[rng.random(z.shape) < 0.01] = nodata if not np.isnan(nodata) else np.nan
    if dtype != np.int16:
        z[40, 100:120] = np.nan
    return z.astype(dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32, np.int16), ids=("f64", "f32", "i16"))
def test_plane_types_with_a_nodata_value_and_nan_and_every_predicate(hip, dtype):
    for nodata in ((-32768.0,) if dtype == np.int16 else (-32768.0, NAN)):
        z = _typed(dtype, nodata)
        st = _stack(hip, z[None], nodata)
        for where in pr.WHERE:
            thr = None if where in ("na", "valid") else 7.0
            got, info = _run(hip, st, where=where, threshold=thr, value_layer=0)
            want = pr.proximity(z, nodata, where, thr, unit=UNIT, value_plane=z)
            for k in ALL:
                assert _same(got[k], want[k]), (dtype, nodata, where, k)
            assert info["n_features"] == pr.features(z, nodata, where, thr).sum() > 0


def test_padded_stack_with_a_layer_and_a_value_layer_and_float32_products(hip):
    import torch
    rng = np.random.default_rng(23)
    z = rng.integers(0, 50, (3, 67, 129)).astype(np.float32)
    z[2][rng.random((67, 129)) < 0.2] = np.nan
    st = _stack(hip, z, pad=7)
    got, _ = _run(hip, st, layer=1, where="lt", threshold=1.0, value_layer=2, out_dtype=torch.float32)
    want = pr.proximity(z[1], None, "lt", 1.0, unit=UNIT, value_plane=z[2], f32=True)
    for k in ALL:
        assert _same(got[k], want[k]), k
    assert got["dist"].dtype == np.float32 and np.isnan(got["value"]).any() and not np.isnan(got["value"]).all()
    # an explicit unit; one product comes back as the tensor itself; a subset of the products
    d, _ = hip.proximity.proximity(st, 1, "lt", 1.0, "dist", unit=0.1)
    assert _same(d.cpu().numpy(), pr.proximity(z[1], None, "lt", 1.0, unit=0.1)["dist"])
    sub, _ = _run(hip, st, layer=1, where="lt", threshold=1.0, products=("dir_y", "d2"))
    assert list(sub) == ["dir_y", "d2"] and _same(sub["d2"], want["d2"]) and _same(sub["dir_y"].astype(np.float32), want["dir_y"])


@pytest.mark.parametrize("shape, at", (((1, 46000), (0, 0)), ((1, 46000), (0, 45999)), ((46000, 1), (0, 0)), ((46000, 1), (45999, 0))),
                         ids=("row_first", "row_last", "col_first", "col_last"))
def test_d2_just_under_the_int32_limit(hip, shape, at):
    mask = np.zeros(shape, bool); mask[at] = True
    z = np.where(mask, np.nan, 2.0)[None]
    got, info = _run(hip, _stack(hip, z), where="na", value_layer=0)
    d2, idx = pr.brute(mask)                                        # one feature: one step
    want = pr.products(d2, idx, shape[1], UNIT, z[0])
    assert want["d2"].max() == 2115908001 == info["max_d2"] and info["n_features"] == 1
    for k in ALL:
        assert _same(got[k], want[k]), k


def test_host_entry_bool_tensor_and_repeat_give_the_same_bytes(hip):
    import torch
    from machisplin_amd import _lib
    mask = masks(67, 129)["random0.05"]
    z = _mask_layers(mask)
    st = _stack(hip, z)
    got, info = _run(hip, st, where="na", value_layer=1)
    again, _ = _run(hip, st, where="na", value_layer=1)
    for k in ALL:
        assert got[k].tobytes() == again[k].tobytes(), k
    # the host-pointer form
    host = {k: np.empty((67, 129), dtype=np.int32 if k in ("d2", "index") else np.float64) for k in ALL}
    out = _lib.ProximityOut(*[host[k].ctypes.data for k in ALL])
    hinfo = _lib.ProximityInfo()
    g = st.geom.c_struct()
    s = _lib.Stack(z.ctypes.data, 2, _lib.F64, 67 * 129, 129, NAN)
    _lib.check(_lib.lib().mhs_proximity(C.byref(g), C.byref(s), 0, 0, 0.0, 1, UNIT, C.byref(out), _lib.F64, C.byref(hinfo)))
    for k in ALL:
        assert _same(host[k], got[k]), k
    assert hinfo.n_features == info["n_features"] == mask.sum() and hinfo.max_d2 == info["max_d2"]
    # the value layer may be the feature layer; float32 planes come down as float32
    h32 = np.empty((67, 129), dtype=np.float32)
    out = _lib.ProximityOut(None, None, None, None, None, h32.ctypes.data)
    _lib.check(_lib.lib().mhs_proximity(C.byref(g), C.byref(s), 1, 1, 0.0, 1, UNIT, C.byref(out), _lib.F32, None))
    assert _same(h32, pr.proximity(z[1], None, "valid", value_plane=z[1], f32=True)["value"])
    # a tensor of flags in the place of the stack: bool and integer, unit 1
    for flags in (torch.from_numpy(mask), torch.from_numpy(mask.astype(np.int16) * 3), torch.from_numpy(mask.astype(np.int64)).cuda()):
        planes, binfo = hip.proximity.proximity(flags, products=("d2", "index", "dist"))
        assert _same(planes["d2"].cpu().numpy(), got["d2"]) and _same(planes["index"].cpu().numpy(), got["index"])
        assert _same(planes["dist"].cpu().numpy(), np.sqrt(got["d2"].astype(np.float64)))
        assert binfo["n_features"] == mask.sum()


def _dem(hip):
    """a 60 x 80 valley system sloping to a sea of NA cells in the south-east, 30 m cells"""
    r, c = np.meshgrid(np.arange(60.0), np.arange(80.0), indexing="ij")
    rng = np.random.default_rng(31)
    z = 200.0 - 1.5 * r - 1.0 * c + 15.0 * np.sin(c / 6.0) * np.cos(r / 9.0) + rng.standard_normal((60, 80))
    z[r + c > 115] = np.nan
    return z, _stack(hip, z[None].astype(np.float32))


def test_covariates_distance_entries(hip):
    import torch
    from machisplin_amd import terrain
    z, st = _dem(hip)
    prox = hip.proximity.proximity
    cov = terrain.covariates(st, ("dist_na", ("dist_le", 100), ("dist_ge", 150.5), "slope_deg"))
    assert cov.names == ["dem", "dist_na", "dist_le100", "dist_ge150.5", "slope_deg"] and cov.planes.dtype == torch.float32
    for k, (where, thr) in enumerate((("na", None), ("le", 100.0), ("ge", 150.5)), start=1):
        direct, _ = prox(st, 0, where, thr, "dist", out_dtype=torch.float32)
        assert torch.equal(cov.planes[k].view(torch.int32), direct.view(torch.int32)), where
        want = pr.proximity(st.planes[0].cpu().numpy(), None, where, thr, unit=UNIT, f32=True)["dist"]
        assert _same(cov.planes[k].cpu().numpy(), want)
    # streams: the composition of hydro and proximity, written out
    cov = terrain.covariates(st, (("dist_stream", 30), "twi", ("above_stream", 30), ("dist_stream", 8)))
    assert cov.names == ["dem", "dist_stream30", "twi", "above_stream30", "dist_stream8"]
    hp, _ = terrain.hydro(st, 0, ("twi", "flowacc"))
    dem64 = st.planes[0].to(torch.float64)
    pair = hip.RasterStack(st.geom, torch.stack([hp["flowacc"], dem64]), NAN)
    assert (hp["flowacc"] >= 30).sum() > 0
    for a, k_dist, k_above in ((30.0, 1, 3), (8.0, 4, None)):
        got, _ = prox(pair, 0, "ge", a, ("dist", "value"), value_layer=1)
        assert torch.equal(cov.planes[k_dist].view(torch.int32), got["dist"].to(torch.float32).view(torch.int32)), a
        if k_above:
            above = (dem64 - got["value"]).to(torch.float32)
            assert torch.equal(cov.planes[k_above].view(torch.int32), above.view(torch.int32))
            assert (above[hp["flowacc"] >= a] == 0).all() and torch.isnan(above[torch.isnan(dem64)]).all()
    assert torch.equal(cov.planes[2].view(torch.int32), hp["twi"].to(torch.float32).view(torch.int32))       # the shared hydro call
    # ... and with numpy from the accumulation
    want = pr.proximity(hp["flowacc"].cpu().numpy(), None, "ge", 30.0, unit=UNIT, value_plane=dem64.cpu().numpy())
    assert _same(cov.planes[1].cpu().numpy(), want["dist"].astype(np.float32))
    assert _same(cov.planes[3].cpu().numpy(), (dem64.cpu().numpy() - want["value"]).astype(np.float32))
    with pytest.raises(ValueError, match="dist_stream"):
        terrain.covariates(st, ("dist_stream",))
    with pytest.raises(ValueError, match="dist_le"):
        terrain.covariates(st, ("dist_le",))


def test_covariates_without_the_new_names_are_what_they_were(hip):
    """the stack of a spec that names no distance entry, against the calls the function made before it knew any: byte-identical"""
    import torch
    from machisplin_amd import terrain
    z, st = _dem(hip)
    spec = ("slope_deg", ("above_min", 5), "twi", "log_flowacc", ("geomorphon", 3), "twi_mfd", "eastness", ("svf", 4))
    cov = terrain.covariates(st, spec, lat=45.0)
    assert cov.names == ["dem", "slope_deg", "above_min5", "twi", "log_flowacc", "geomorphon3", "twi_mfd", "eastness", "svf4"]
    tv = terrain.terrain(st, 0, ("slope_deg", "eastness"), out_dtype=torch.float32)
    hp, _ = terrain.hydro(st, 0, ("twi", "flowacc"))
    hm, _ = terrain.hydro_mfd(st, 0, ("twi",))
    geo = terrain.geomorphon(st, 3, 1.0, 0)
    want = [st.planes[0].to(torch.float32), tv[0], terrain.relief(st, 5, "above_min", 0, 1.0, out_dtype=torch.float32), hp["twi"].to(torch.float32),
            torch.log(hp["flowacc"]).to(torch.float32),
            torch.where(geo == terrain.GEOMORPHON_NA, torch.full((), NAN, device=geo.device), geo.to(torch.float32)), hm["twi"].to(torch.float32),
            tv[1], terrain.solar(st, 4, ("svf",), None, 0, False, 45.0, 1.0, out_dtype=torch.float32)[0]]
    for k, w in enumerate(want):
        assert torch.equal(cov.planes[k].view(torch.int32), w.view(torch.int32)), cov.names[k]
