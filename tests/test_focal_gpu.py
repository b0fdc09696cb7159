"""GPU: window statistics at any radius (csrc/focal.hip, machisplin_amd/focal.py) through the C ABI.

1. against the numpy restatement of the section "focal" (tests/focal_ref.py), bit for bit, on float64 planes with full random
   mantissas -- planes made from float32 or from integers sum exactly in any order at these sizes and could not tell one
   summation order from another;
2. independent of the restatement: integer-valued planes, |z| <= 3 000, offset 0 -- every partial sum is an integer below 2^53,
   exact in any order -- against a plain loop over the window's offsets in int64, with the header's formulas, bit for bit;
3. against terrain.relief: the circle's minus_mean at R = 5, 17, 45, bit for bit on integer planes, within the derived bound
   on float64 planes;
4. invariance: a window, the host entry in three bands, three radii in one call, out=, float32 output;
5. the refusals, by name;  6. the covariates() specs.

Planes 70 x 150, 1 x 200, 200 x 1, 3 x 3; radii 1, 2, B - 1, B, B + 1, 2 B + 2 and one that covers the raster from any cell; an NA
cluster, an all-NA row, nodata and NaN."""
import ctypes as C
import functools

import numpy as np
import pytest

import focal_ref as fr

pytestmark = pytest.mark.gpu

B = fr.B
NODATA = -32768.0
SHAPES = ((70, 150), (1, 200), (200, 1), (3, 3))
RADII = (1, 2, B - 1, B, B + 1, 2 * B + 2, 200)
SUMS = ("count", "sum", "mean", "sd", "minus_mean", "dev")


def _radii(shape):
    return tuple(R for R in RADII if R <= max(shape))


def _geom(shape):
    from machisplin_amd import Geometry
    return Geometry(500000.0, 4100000.0, 30.0, 30.0, *shape)


@functools.lru_cache(maxsize=None)
def _plane(shape, kind):
    """kind "full": float64 with full random mantissas around 2 000 +- 300; "int": integer-valued float64, |z| <= 3 000; "f32", "i16":
    that plane type.  An NA cluster, an all-NA row (where the plane has more than three), NaN and the nodata value."""
    nr, nc = shape
    rng = np.random.default_rng(1000 * nr + nc + {"full": 0, "int": 1, "f32": 2, "i16": 3}[kind])
    r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
    z = 2000.0 + 1.5 * r - 0.7 * c + 300.0 * rng.standard_normal(shape) * rng.random(shape)
    if kind == "int":
        z = np.rint(np.clip(z - 2000.0, -3000.0, 3000.0))
    elif kind == "i16":
        z = np.rint(z).astype(np.int16)
    elif kind == "f32":
        z = z.astype(np.float32)
    na = np.zeros(shape, dtype=bool)
    if nr > 3:
        na[nr // 3] = True                                         # an all-NA row
        na[nr // 2:nr // 2 + 5, nc // 4:nc // 4 + 9] = True         # a cluster
    na |= rng.random(shape) < 0.03
    if nr * nc <= 9:
        na[:] = False
        na[0, 1] = True
    z = z.copy()
    if kind == "i16":
        z[na] = np.int16(NODATA)
    else:
        z[na & (rng.random(shape) < 0.5)] = NODATA
        z[na & (z != NODATA)] = np.nan
    z.setflags(write=False)
    return z


def _stack(hip, shape, kind):
    return hip.RasterStack(_geom(shape), np.array(_plane(shape, kind)[None]), NODATA)


def _same(got, want):
    """bit for bit: the same values, NaN where it is NaN, the same sign of zero"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got) & ~np.isnan(got), np.signbit(want) & ~np.isnan(want))


# ---------------------------------------------------------------- 1. the restatement

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("window_shape", ("square", "circle"))
def test_every_statistic_equals_the_restatement_bit_for_bit(hip, shape, window_shape):
    from machisplin_amd import focal
    stack = _stack(hip, shape, "full")
    z = _plane(shape, "full")
    off = 2000.0
    for R in _radii(shape):
        for fill in (False, True):
            names = SUMS if window_shape == "circle" else fr.STATS
            got = focal.focal(stack, R, names, shape=window_shape, fill_na=fill, offset=off).cpu().numpy()
            want = fr.focal(z, NODATA, R, names, window_shape, fill, off)
            assert _same(got, want), (R, fill, [k for k, (a, b) in zip(names, zip(got, want)) if not _same(a, b)])
            na = np.isnan(z) | (z == NODATA)
            centre = [k for k, name in enumerate(names) if name in ("minus_mean", "above_min", "below_max", "dev")]
            assert na.any() and np.isnan(got[centre][:, na]).all()              # these need the centre
            assert not np.isnan(got[0][na]).any() if fill else np.isnan(got[:, na]).all()
    # the restatement can tell orders apart on these planes: a plain sequential row-major sum differs somewhere
    if shape == (70, 150):
        n, S1, _, _, _ = fr.brute(z, NODATA, 2, window_shape, off)
        assert not np.array_equal(S1, fr.sums(z, NODATA, 2, window_shape, off)[1])


@pytest.mark.parametrize("kind", ("f32", "i16"))
def test_plane_types_and_nodata(hip, kind):
    from machisplin_amd import focal
    shape = (70, 150)
    stack = _stack(hip, shape, kind)
    z = _plane(shape, kind).astype(np.float64)
    for R, ws in ((2, "square"), (B + 1, "square"), (5, "circle")):
        names = SUMS if ws == "circle" else fr.STATS
        got = focal.focal(stack, R, names, shape=ws, fill_na=True, offset=1999.0).cpu().numpy()
        assert _same(got, fr.focal(z, NODATA, R, names, ws, True, 1999.0)), (R, ws)


def test_default_offset_is_the_rounded_mean(hip):
    from machisplin_amd import focal
    shape = (70, 150)
    stack = _stack(hip, shape, "full")
    z, ok = fr.valid(_plane(shape, "full"), NODATA)
    off = focal.default_offset(stack)
    assert off == np.rint(off) and abs(off - z[ok].mean()) <= 0.5 + 1e-6
    got = focal.focal(stack, 7, "sd").cpu().numpy()
    assert _same(got, fr.focal(z, NODATA, 7, ("sd",), "square", False, off)[0])


# ---------------------------------------------------------------- 2. independent of the restatement

def _offset_loop(z, nodata, R):
    """(n, S1, S2, min, max) of the square window by a loop over the window's offsets, the sums in int64: exact on integer planes"""
    z, ok = fr.valid(z, nodata)
    zi = np.where(ok, z, 0.0).astype(np.int64)
    nr, nc = z.shape
    n, S1, S2 = (np.zeros(z.shape, dtype=np.int64) for _ in range(3))
    mn, mx = np.full(z.shape, np.inf), np.full(z.shape, -np.inf)
    for dr in range(-min(R, nr - 1), min(R, nr - 1) + 1):
        for dc in range(-min(R, nc - 1), min(R, nc - 1) + 1):
            dst = (slice(max(0, -dr), min(nr, nr - dr)), slice(max(0, -dc), min(nc, nc - dc)))
            src = (slice(max(0, dr), min(nr, nr + dr)), slice(max(0, dc), min(nc, nc + dc)))
            n[dst] += ok[src]
            S1[dst] += zi[src]
            S2[dst] += zi[src] * zi[src]
            mn[dst] = np.minimum(mn[dst], np.where(ok[src], z[src], np.inf))
            mx[dst] = np.maximum(mx[dst], np.where(ok[src], z[src], -np.inf))
    return n, S1.astype(np.float64), S2.astype(np.float64), mn, mx


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_planes_equal_a_plain_window_loop_bit_for_bit(hip, shape):
    from machisplin_amd import focal
    stack = _stack(hip, shape, "int")
    z, ok = fr.valid(_plane(shape, "int"), NODATA)
    names = ("count", "sum", "mean", "sd", "min", "max", "range")
    for R in _radii(shape):
        n, S1, S2, mn, mx = _offset_loop(z, NODATA, R)
        assert S2.max() < 2.0 ** 53
        want = fr.statistics(n, S1, S2, z, ok, 0.0, True, mn, mx)
        got = focal.focal(stack, R, names, fill_na=True, offset=0.0).cpu().numpy()
        for k, name in enumerate(names):
            assert _same(got[k], want[name]), (R, name)


# ---------------------------------------------------------------- 3. against terrain.relief

@pytest.mark.parametrize("R", (5, 17, 45))
def test_circle_minus_mean_against_relief(hip, R):
    from machisplin_amd import focal, terrain
    shape = (70, 150)
    stack = _stack(hip, shape, "int")
    got = focal.focal(stack, R, "minus_mean", shape="circle", offset=0.0).cpu().numpy()
    want = terrain.relief(stack, R, "minus_mean", z_factor=1.0).cpu().numpy()
    assert _same(got, want)
    # float64 planes: the two sums are the same numbers added in two orders
    stack = _stack(hip, shape, "full")
    z, ok = fr.valid(_plane(shape, "full"), NODATA)
    got = focal.focal(stack, R, ("minus_mean", "count"), shape="circle", offset=0.0).cpu().numpy()
    want = terrain.relief(stack, R, "minus_mean", z_factor=1.0).cpu().numpy()
    assert np.array_equal(np.isnan(got[0]), np.isnan(want)) and not np.isnan(want[ok]).any()
    n = got[1][ok]
    n_max = (2 * R + 1) ** 2
    A = np.abs(z[ok]).sum()
    # |sum_focal - S| <= the header's bound; |sum_relief - S| <= n u / (1 - n u) A (a sequential sum of n terms); each mean = one
    # division (relative u) and focal's 0 + S1 / n adds nothing; the difference e - mean is rounded once in both
    tol = (fr.bound(z, NODATA, R, "circle", 0.0) + 1.01 * n_max * fr.U * A) / n + 4.0 * fr.U * (np.abs(z[ok]) + np.abs(want[ok]))
    err = np.abs(got[0][ok] - want[ok])
    print(f"R = {R}: max |focal - relief| = {err.max():.3e}, smallest tolerance {tol.min():.3e}")
    assert (err <= tol).all()


# ---------------------------------------------------------------- 4. invariance

def test_window_radii_out_and_float32(hip):
    import torch
    from machisplin_amd import focal
    shape = (70, 150)
    stack = _stack(hip, shape, "full")
    for ws, radii in (("square", (2, B + 1, 2 * B + 2)), ("circle", (3, 17, B + 1))):
        names = ("mean", "sd", "count", "dev") if ws == "circle" else ("mean", "range", "count", "below_max")
        singles = [focal.focal(stack, R, names, shape=ws, offset=2000.0) for R in radii]
        many = focal.focal(stack, radii, names, shape=ws, offset=2000.0)
        assert many.shape == (3, 4) + shape
        for k in range(3):
            assert _same(many[k].cpu().numpy(), singles[k].cpu().numpy()), (ws, radii[k])
        win = (3, 69, 5, 133)                                      # origins that are no multiple of B or of the tile
        part = focal.focal(stack, radii, names, shape=ws, offset=2000.0, window=win).cpu().numpy()
        assert _same(part, many.cpu().numpy()[:, :, 3:69, 5:133]), ws
        out = torch.full((12,) + shape, 7.0, dtype=torch.float64, device="cuda")
        res = focal.focal(stack, radii, names, shape=ws, offset=2000.0, out=out)
        lib_order = sorted(names, key=focal.STATS.index)
        for k in range(3):
            for j, name in enumerate(lib_order):
                assert _same(out[4 * k + j].cpu().numpy(), singles[k][names.index(name)].cpu().numpy())
        assert _same(res.cpu().numpy(), many.cpu().numpy())
        f32 = focal.focal(stack, radii[1], names, shape=ws, offset=2000.0, out_dtype=torch.float32).cpu().numpy()
        assert f32.dtype == np.float32 and np.array_equal(f32, singles[1].cpu().numpy().astype(np.float32), equal_nan=True)
    one = focal.focal(stack, 4, "mean", offset=2000.0)
    assert one.shape == shape and _same(one.cpu().numpy(), focal.focal(stack, [4], ("mean",), offset=2000.0)[0, 0].cpu().numpy())


@pytest.mark.parametrize("ws", ("square", "circle"))
def test_host_entry_in_three_bands(hip, ws, monkeypatch):
    from machisplin_amd import _lib, focal
    shape = (200, 70)
    z = np.ascontiguousarray(_plane((70, 200), "full").T)          # 200 rows: bands of 67 rows, more than a block
    stack = hip.RasterStack(_geom(shape), z[None], NODATA)
    radii = (2, B + 1, 150)
    names = ("count", "sum", "sd") if ws == "circle" else ("count", "sum", "sd", "min", "max")
    mask = sum(1 << focal.STATS.index(k) for k in names)
    win = (5, 197, 3, 66)
    want = focal.focal(stack, radii, names, shape=ws, fill_na=True, offset=2000.0, window=win).cpu().numpy().reshape(3 * len(names), 192, 63)
    g = _geom(shape).c_struct()
    st = _lib.Stack(z.ctypes.data, 1, _lib.F64, z.size, shape[1], NODATA)
    rad = (C.c_int * 3)(*radii)
    for bands in ("3", None):
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)
        else:
            monkeypatch.delenv("MHS_HOST_BANDS")
        out = np.zeros((3 * len(names), 192, 63))
        rc = _lib.lib().mhs_focal(C.byref(g), C.byref(st), 0, rad, 3, focal.SHAPES.index(ws), mask, 1, 2000.0, *win, out.ctypes.data, _lib.F64)
        assert rc == _lib.OK, _lib.lib().mhs_last_error()
        assert _same(out, want), bands


# ---------------------------------------------------------------- 5. refusals

def test_refusals_name_the_argument(hip):
    import torch
    from machisplin_amd import MhsError, focal
    shape = (70, 150)
    stack = _stack(hip, shape, "full")
    with pytest.raises(MhsError, match=r"radius must be in 1 \.\. 150 .*radii\[0\] = 0"):
        focal.focal(stack, 0, "mean")
    with pytest.raises(MhsError, match=r"radius must be in 1 \.\. 150 .*radii\[1\] = 151"):
        focal.focal(stack, (3, 151), "mean")
    with pytest.raises(ValueError, match="1 .. 8 radii"):
        focal.focal(stack, list(range(1, 10)), "mean")
    with pytest.raises(ValueError, match="relief.*square"):
        focal.focal(stack, 3, "max", shape="circle")
    with pytest.raises(ValueError, match="unknown statistic 'median'"):
        focal.focal(stack, 3, "median")
    with pytest.raises(ValueError, match="unknown shape"):
        focal.focal(stack, 3, "mean", shape="ring")
    with pytest.raises(MhsError, match="layer 1 is not one of"):
        focal.focal(stack, 3, "mean", layer=1, offset=0.0)
    with pytest.raises(ValueError, match="out must be"):
        focal.focal(stack, 3, "mean", out=torch.zeros((2,) + shape, dtype=torch.float64, device="cuda"))
    # the C entry itself
    from machisplin_amd import _lib
    g, s = stack.geom.c_struct(), stack.c_struct()
    out = torch.zeros(shape, dtype=torch.float64, device="cuda")
    call = lambda radii, n, ws, mask, off=0.0: _lib.lib().mhs_focal_dev(C.byref(g), C.byref(s), 0, (C.c_int * 9)(*radii), n, ws, mask, 0, off, 0, 70, 0, 150,
                                                                       out.data_ptr(), _lib.F64, 150, 70 * 150, None)
    for args, text in ((((1,) * 9, 9, 0, 4), "n_radii must be in 1 .. 8"), (((1,) * 9, 0, 0, 4), "n_radii"), (((1,) * 9, 1, 1, 1 << 5), "circle window gives the sum family"),
                       (((1,) * 9, 1, 2, 4), "shape must be"), (((1,) * 9, 1, 0, 1 << 11), "unknown bits"), (((1,) * 9, 1, 0, 0), "selects nothing"),
                       (((1,) * 9, 1, 0, 4, float("inf")), "offset must be finite")):
        assert call(*args) == _lib.ERR_INVALID and text in _lib.lib().mhs_last_error().decode(), text
    assert (out == 0).all()


# ---------------------------------------------------------------- 6. covariates

def test_covariates_specs(hip):
    import torch
    from machisplin_amd import focal, terrain
    shape = (70, 150)
    stack = _stack(hip, shape, "full")
    spec = (("focal_mean", 70), ("tpi_scale", 70), ("focal_sd", 5), ("dev", 70), "slope_deg", ("above_min", 17))
    cov = terrain.covariates(stack, spec)
    assert cov.names == ["dem", "focal_mean70", "tpi_scale70", "focal_sd5", "dev70", "slope_deg", "above_min17"]
    off = focal.default_offset(stack)
    want = {R: focal.focal(stack, R, ("mean", "sd", "minus_mean", "dev"), out_dtype=torch.float32, offset=off).cpu().numpy() for R in (70, 5)}
    got = cov.planes.cpu().numpy()
    for k, (name, R) in enumerate((("mean", 70), ("minus_mean", 70), ("sd", 5), ("dev", 70))):
        assert np.array_equal(got[1 + k], want[R][("mean", "sd", "minus_mean", "dev").index(name)], equal_nan=True), (name, R)
    # the specs that were there give the planes they gave: those of the direct calls
    old = terrain.covariates(stack, ("slope_deg", ("above_min", 17), ("minus_mean", 45))).planes.cpu().numpy()
    assert np.array_equal(old[1], terrain.terrain(stack, 0, "slope_deg", out_dtype=torch.float32).cpu().numpy(), equal_nan=True)
    assert np.array_equal(old[2], terrain.relief(stack, 17, "above_min", out_dtype=torch.float32).cpu().numpy(), equal_nan=True)
    assert np.array_equal(old[3], terrain.relief(stack, 45, "minus_mean", out_dtype=torch.float32).cpu().numpy(), equal_nan=True)
    assert np.array_equal(got[5], old[1], equal_nan=True) and np.array_equal(got[6], old[2], equal_nan=True)
    with pytest.raises(_lib_error(), match="radius must be in 1 .. 45"):
        terrain.covariates(stack, (("above_min", 46),))
    with pytest.raises(ValueError, match="takes one argument, the radius"):
        terrain.covariates(stack, (("focal_mean", 3, 4),))


def _lib_error():
    from machisplin_amd import MhsError
    return MhsError
