"""GPU: connected patches (include/machisplin_hip.h, section "patches"; csrc/patches.hip).  All five products -- label, id, size,
edge, keep -- and the info's counts equal the flood-fill restatement of tests/patches_ref.py exactly.

Shapes: the degenerate ones, every combination of one less than, exactly and one more than a tile in the two dimensions
(PATCH_TILE_ROWS, PATCH_TILE_COLS, read from the text of csrc/patches_rule.h), and 2 x 2 tiles and a bit, so that there are
interior tile corners.  Each shape is crossed with both connectivities and the masks that stress the union-find: nothing,
everything (one patch through every tile), a checkerboard (one patch at 8; every cell its own at 4: the largest patch count),
the two diagonals through the tile corners (the SE / SW corner links), one-cell-wide serpentines that cross every tile border
many times (the longest pointer chains), a comb whose teeth join only in the last row (the smallest cell number is learnt
last), and random masks at the two percolation thresholds.

scratch_bytes: the rule's 12 bytes per cell are the per-cell planes (label 4, counts 4, ids 4); the block also holds parts
the header names apart from them -- five sub-blocks each padded to 256 bytes, and 4 bytes per PATCH_SCAN_BLOCK cells -- which
scratch_bound() adds: on a 1 x 1 plane the counters alone are more than 12 bytes.  Where label is written in place and the
plane has more than a few hundred cells, the plain bound of 12 bytes per cell is asserted."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import patches_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
ALL = pr.PRODUCTS


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "patches_rule.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


TR, TC, SCAN = _constant("PATCH_TILE_ROWS"), _constant("PATCH_TILE_COLS"), _constant("PATCH_SCAN_BLOCK")
SHAPES = [(1, 1), (1, TC + 1), (TR + 1, 1)] + [(r, c) for r in (TR - 1, TR, TR + 1) for c in (TC - 1, TC, TC + 1)] + [(2 * TR + 3, 2 * TC + 5)]


STEP = math.gcd(TR, TC)                # (a TR - 1, b TC - 1) and (a TR, b TC) lie on one diagonal of this spacing, whatever a and b
SCRATCH_FIXED = 5 * 256                # label, counts, ids, block counts, counters: each sub-block is padded to 256 bytes


def scratch_bound(n):
    return 12 * n + SCRATCH_FIXED + 4 * (n // SCAN + 1)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def masks(nrow, ncol):
    """name -> boolean feature mask"""
    rng = np.random.default_rng(nrow * 1000 + ncol)
    r, c = np.meshgrid(np.arange(nrow), np.arange(ncol), indexing="ij")
    out = {"none": np.zeros((nrow, ncol), bool), "all": np.ones((nrow, ncol), bool), "checkerboard": (r + c) % 2 == 0,
           "diagonal": (r - c) % STEP == 0, "anti_diagonal": (r + c) % STEP == STEP - 1}   # lines through every corner between four tiles
    m = r % 2 == 0                                                       # full rows, joined at alternating ends
    m |= (r % 4 == 1) & (c == ncol - 1)
    m |= (r % 4 == 3) & (c == 0)
    out["serpentine_rows"] = m
    m = c % 2 == 0                                                       # full columns, joined at alternating ends
    m |= (c % 4 == 1) & (r == nrow - 1)
    m |= (c % 4 == 3) & (r == 0)
    out["serpentine_cols"] = m
    out["comb"] = (c % 2 == 0) | (r == nrow - 1)
    for d in (0.41, 0.59):
        for seed in range(3):
            out[f"random{d:g}_{seed}"] = rng.random((nrow, ncol)) < d
    return out


_REF = {}


def reference(shape, name, conn):
    """the restatement's planes and counts of one mask, computed once (filter: 2 <= size <= 40, any edge)"""
    key = (shape, name, conn)
    if key not in _REF:
        _REF[key] = pr.patches(masks(*shape)[name], conn, 2, 40)
    return _REF[key]


def _stack(hip, layers, nodata=NAN, pad=0):
    """a RasterStack; pad > 0: cut out of a tensor with `pad` more columns and one more layer"""
    import torch
    layers = np.asarray(layers)
    n, nr, nc = layers.shape
    st = hip.RasterStack(hip.Geometry(1000.0, 5000.0, 30.0, 30.0, nr, nc), layers, nodata)
    if pad:
        big = torch.full((n + 1, nr, nc + pad), 5, dtype=st.planes.dtype, device=st.planes.device)
        big[1:, :, :nc] = st.planes
        st.planes = big[1:, :, :nc]
        assert st.planes.stride(1) == nc + pad
    return st


def _run(hip, stack, **kw):
    kw.setdefault("products", ALL)
    planes, info = hip.patches.patches(stack, **kw)
    return {k: v.cpu().numpy() for k, v in planes.items()}, info


def _check(got, info, want, winfo, tag):
    for k in ALL:
        assert _same(got[k], want[k]), (tag, k)
    for k, v in winfo.items():
        assert info[k] == v, (tag, k, info[k], v)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_product_on_every_mask_equals_the_restatement(hip, shape, conn):
    import torch
    for name, mask in masks(*shape).items():
        want, winfo = reference(shape, name, conn)
        got, info = _run(hip, torch.from_numpy(mask), connectivity=conn, min_size=2, max_size=40)
        _check(got, info, want, winfo, (shape, name, conn))
        assert info["scratch_bytes"] <= (12 * mask.size if mask.size >= 512 else scratch_bound(mask.size)), (shape, name)
        if name == "none":
            assert (got["label"] == -1).all() and all((got[k] == 0).all() for k in ALL[1:]) and info["max_size"] == 0
        if name == "checkerboard":
            assert info["n_patches"] == (1 if conn == 8 and min(shape) > 1 else mask.sum())       # one row or column has no diagonal
        if name in ("all", "serpentine_rows", "serpentine_cols", "comb"):
            assert info["n_patches"] == 1 and (got["label"][mask] == 0).all() and info["max_size"] == mask.sum()


def test_large_random_mask_equals_scipy_canonically_relabelled(hip):
    ndi = pytest.importorskip("scipy.ndimage")
    import torch
    mask = np.random.default_rng(41).random((1500, 1700)) < 0.5
    flags = torch.from_numpy(mask).cuda()
    for conn, structure in ((8, np.ones((3, 3))), (4, None)):
        lab, k = ndi.label(mask, structure=structure)
        first = np.unique(lab.ravel(), return_index=True)[1]           # the first cell of id 0 (the background), 1, 2, ...: the smallest
        first[0] = -1
        want, winfo = pr.products(first[lab], 3, None, "interior")
        got, info = _run(hip, flags, connectivity=conn, min_size=3, edge="interior")
        assert np.array_equal(got["id"], lab) and info["n_patches"] == k
        _check(got, info, want, winfo, conn)
        assert info["scratch_bytes"] <= 12 * mask.size                  # here without the allowance: label is written in place


def test_crop_of_the_large_mask_equals_the_flood_fill(hip):
    """more than a few tiles against the restatement itself, so that a machine without scipy checks them too"""
    import torch
    mask = (np.random.default_rng(41).random((1500, 1700)) < 0.5)[:300, :340]
    for conn in (4, 8):
        want, winfo = pr.patches(mask, conn, 1, 1000, "touching")
        got, info = _run(hip, torch.from_numpy(mask.copy()), connectivity=conn, max_size=1000, edge="touching")
        _check(got, info, want, winfo, conn)


def _typed(dtype, nodata):
    """a 67 x 133 plane of the type: small whole values, NA in clusters as the nodata value (and NaN in float planes)"""
    rng = np.random.default_rng(17)
    z = rng.integers(-3, 40, (2 * TR + 3, 2 * TC + 5)).astype(np.float64)
    na = nodata if not np.isnan(nodata) else np.nan
    z[10:14, 20:90] = na
    z[30:36, 60:70] = na                                                # across the corner of four tiles
    z[rng.random(z.shape) < 0.05] = na
    if dtype != np.int16:
        z[40, 100:120] = np.nan
    return z.astype(dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32, np.int16), ids=("f64", "f32", "i16"))
def test_plane_types_with_a_nodata_value_and_two_predicates(hip, dtype):
    for nodata in ((-32768.0,) if dtype == np.int16 else (-32768.0, NAN)):
        z = _typed(dtype, nodata)
        st = _stack(hip, z[None], nodata)
        for where, thr in (("na", None), ("ge", 20.0), ("valid", None)):
            mask = pr.features(z, nodata, where, thr)
            for conn in (4, 8):
                want, winfo = pr.patches(mask, conn, 2, None, "interior")
                got, info = _run(hip, st, where=where, threshold=thr, connectivity=conn, min_size=2, edge="interior")
                _check(got, info, want, winfo, (dtype, nodata, where, conn))
                assert winfo["n_features"] > 0


def test_strided_stack_stream_subsets_host_entry_and_repeat(hip):
    import torch
    from machisplin_amd import _lib
    shape = (2 * TR + 3, 2 * TC + 5)
    n = shape[0] * shape[1]
    rng = np.random.default_rng(23)
    z = rng.integers(0, 50, (3,) + shape).astype(np.float32)
    st = _stack(hip, z, pad=7)
    mask = z[1] < 21.0
    want, winfo = pr.patches(mask, 8, 4, 60, "touching")
    kw = dict(layer=1, where="lt", threshold=21.0, min_size=4, max_size=60, edge="touching")
    got, info = _run(hip, st, **kw)
    _check(got, info, want, winfo, "padded")
    # the same call made twice gives identical bytes
    again, info2 = _run(hip, st, **kw)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ALL) and info == info2
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        planes, sinfo = hip.patches.patches(st, products=ALL, stream=side.cuda_stream, **kw)
    side.synchronize()
    assert all(_same(planes[k].cpu().numpy(), want[k]) for k in ALL) and sinfo == info
    # a single product comes back as the tensor itself; subsets in the caller's order; the label plane in scratch: 12 bytes per cell
    lab, linfo = hip.patches.patches(st, products="label", **kw)
    assert isinstance(lab, torch.Tensor) and _same(lab.cpu().numpy(), want["label"]) and linfo["n_patches"] == winfo["n_patches"]
    sub, subinfo = _run(hip, st, products=("keep", "id", "size"), **kw)
    assert list(sub) == ["keep", "id", "size"] and all(_same(sub[k], want[k]) for k in sub)
    assert 12 * n <= subinfo["scratch_bytes"] <= scratch_bound(n) and info["scratch_bytes"] < subinfo["scratch_bytes"]
    for name in ALL[1:]:
        one, _ = hip.patches.patches(st, products=name, **kw)
        assert _same(one.cpu().numpy(), want[name]), name
    keep = hip.patches.sieve(st, **kw)
    assert _same(keep.cpu().numpy(), want["keep"])
    # a tensor of flags in the place of the stack: bool and integer, host or device
    for flags in (torch.from_numpy(mask), torch.from_numpy(mask.astype(np.int16) * 3), torch.from_numpy(mask.astype(np.int64)).cuda()):
        p, finfo = _run(hip, flags, min_size=4, max_size=60, edge="touching")
        _check(p, finfo, want, winfo, "flags")
    # the host-pointer form
    host = {k: np.empty(shape, dtype=want[k].dtype) for k in ALL}
    out = _lib.PatchesOut(*[host[k].ctypes.data for k in ALL])
    hinfo = _lib.PatchesInfo()
    g = st.geom.c_struct()
    s = _lib.Stack(z.ctypes.data, 3, _lib.F32, n, shape[1], NAN)
    _lib.check(_lib.lib().mhs_patches(C.byref(g), C.byref(s), 1, 2, 21.0, 8, 4, 60, 1, C.byref(out), C.byref(hinfo)))
    assert all(_same(host[k], want[k]) for k in ALL)
    assert all(getattr(hinfo, k) == v for k, v in winfo.items())
    # the device entry with a row stride of its own and without info: label goes through the scratch and is copied out
    wide = torch.full((5, shape[0], shape[1] + 3), 77, dtype=torch.int32, device="cuda")
    src = st.planes
    cs = _lib.Stack(src.data_ptr(), 3, _lib.F32, src.stride(0), src.stride(1), NAN)
    out = _lib.PatchesOut(wide[0].data_ptr(), wide[1].data_ptr(), None, None, None)
    _lib.check(_lib.lib().mhs_patches_dev(C.byref(g), C.byref(cs), 1, 2, 21.0, 8, 4, 60, 1, C.byref(out), shape[1] + 3,
                                          torch.cuda.current_stream().cuda_stream, None))
    torch.cuda.synchronize()
    w = wide.cpu().numpy()
    assert np.array_equal(w[0, :, :shape[1]], want["label"]) and np.array_equal(w[1, :, :shape[1]], want["id"])
    assert (w[:2, :, shape[1]:] == 77).all() and (w[2:] == 77).all()


def _dem(hip):
    """a 60 x 80 valley system sloping to a sea of NA cells in the south-east, with voids and a masked lake inland, 30 m cells"""
    r, c = np.meshgrid(np.arange(60.0), np.arange(80.0), indexing="ij")
    rng = np.random.default_rng(31)
    z = 200.0 - 1.5 * r - 1.0 * c + 15.0 * np.sin(c / 6.0) * np.cos(r / 9.0) + rng.standard_normal((60, 80))
    z[r + c > 115] = np.nan
    z[10, 10:13] = np.nan                                               # a void of three cells
    z[30:34, 20:25] = np.nan                                            # a lake of twenty
    z[5, 40] = np.nan
    return z, _stack(hip, z[None].astype(np.float32))


def test_covariates_patch_distance_entries(hip):
    import torch
    from machisplin_amd import terrain
    z, st = _dem(hip)
    prox, sieve = hip.proximity.proximity, hip.patches.sieve
    cov = terrain.covariates(st, ("dist_na_edge", ("dist_na_min", 4), ("dist_na_min", 21), ("dist_le_min", 100, 30), "dist_na", "slope_deg"))
    assert cov.names == ["dem", "dist_na_edge", "dist_na_min4", "dist_na_min21", "dist_le100_min30", "dist_na", "slope_deg"]
    assert cov.planes.dtype == torch.float32
    keeps = (sieve(st, 0, "na", None, 8, edge="touching"), sieve(st, 0, "na", None, 8, min_size=4), sieve(st, 0, "na", None, 8, min_size=21),
             sieve(st, 0, "le", 100.0, 8, min_size=30))
    z32 = st.planes[0].cpu().numpy()
    masks_ = (pr.features(z32, None, "na"), pr.features(z32, None, "na"), pr.features(z32, None, "na"), pr.features(z32, None, "le", 100.0))
    filt = (dict(edge="touching"), dict(min_size=4), dict(min_size=21), dict(min_size=30))
    import proximity_ref as xr
    for k, (keep, m, f) in enumerate(zip(keeps, masks_, filt), start=1):
        direct, _ = prox(keep, products="dist", unit=30.0, out_dtype=torch.float32)
        assert torch.equal(cov.planes[k].view(torch.int32), direct.view(torch.int32)), cov.names[k]
        kept = pr.patches(m, 8, **f)[0]["keep"]
        assert _same(keep.cpu().numpy(), kept)
        assert _same(cov.planes[k].cpu().numpy(), xr.proximity(kept.astype(np.float64), None, "ne", 0.0, unit=30.0, f32=True)["dist"])
    # the sea alone: the void, the lake and the single cell are no coast; at least 4 cells: the lake counts again
    sea = cov.planes[1].cpu().numpy()
    assert sea[10, 11] > 0 and sea[31, 22] > 0 and sea[5, 40] > 0 and cov.planes[5][10, 11] == 0
    assert cov.planes[2][31, 22] == 0 and cov.planes[2][10, 11] > 0 and cov.planes[3][31, 22] > 0
    assert torch.equal(cov.planes[3].view(torch.int32), cov.planes[1].view(torch.int32))      # only the sea has more than 20 cells
    # the plain entry keeps its bytes
    plain, _ = prox(st, 0, "na", None, "dist", out_dtype=torch.float32)
    assert torch.equal(cov.planes[5].view(torch.int32), plain.view(torch.int32))
    for bad in (("dist_na_min",), ("dist_na_min", 0), ("dist_le_min", 100), ("dist_na_edge", 3)):
        with pytest.raises(ValueError, match=bad[0]):
            terrain.covariates(st, (bad,))
