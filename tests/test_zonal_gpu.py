"""GPU: zonal statistics (include/machisplin_hip.h, section "zonal"; csrc/zonal.hip).  Every table and every plane equals the
numpy and Python-int restatement of tests/zonal_ref.py BIT FOR BIT (the bytes are compared, NaN included), and the info's counts
equal its counts.

Shapes: the degenerate ones, every combination of one less than, exactly and one more than a tile in the two dimensions
(ZONAL_TILE_ROWS, ZONAL_TILE_COLS, read from the text of csrc/zonal_rule.h), and 2 x 2 tiles and a bit.  Each is crossed with
the zone planes that stress the accumulate kernel: one zone everywhere (one hot address; at 67 rows the strip spans tiles),
every cell its own zone (runs of one: the LDS table of ZONAL_LDS_SLOTS slots overflows and the direct path runs), pairs of
cells (more zones in a tile than slots, fewer than cells), one-column and one-row stripes, a checkerboard, no zone at all, and a
zone that occurs in the first and the last tile only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zonal_ref as zr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
ALL, TAB = zr.STATS, zr.TABLE_STATS


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "zonal_rule.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


TR, TC, SLOTS, STRIP = _constant("ZONAL_TILE_ROWS"), _constant("ZONAL_TILE_COLS"), _constant("ZONAL_LDS_SLOTS"), _constant("ZONAL_STRIP_TILES")
BIG = (2 * TR + 3, 2 * TC + 5)
SHAPES = [(1, 1), (1, TC + 1), (TR + 1, 1)] + [(r, c) for r in (TR - 1, TR, TR + 1) for c in (TC - 1, TC, TC + 1)] + [BIG]


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def zone_planes(nrow, ncol):
    """name -> (int32 zone plane, n_zones)"""
    r, c = np.meshgrid(np.arange(nrow), np.arange(ncol), indexing="ij")
    n = nrow * ncol
    cell = r * ncol + c
    ends = np.ones((nrow, ncol), dtype=np.int64)
    ends[0, :3] = 7
    ends[-1, -3:] = 7
    out = {"one": (np.zeros((nrow, ncol)), 1), "own": (cell, n), "pairs": (cell // 2, n // 2 + 1), "columns": (c, ncol), "rows": (r, nrow),
           "checkerboard": ((r + c) % 2, 2), "none": (np.full((nrow, ncol), -1), 3), "ends": (ends, 9)}
    return {k: (z.astype(np.int32), nz) for k, (z, nz) in out.items()}


def values(nrow, ncol, dtype):
    """(plane, nodata): random values with NA; the float32 ones are not multiples of the default quantum"""
    rng = np.random.default_rng(nrow * 1000 + ncol)
    if dtype == np.int16:
        v = rng.integers(-500, 9000, (nrow, ncol)).astype(np.int16)
        v[rng.random((nrow, ncol)) < 0.1] = -32768
        return v, -32768.0
    v = (100.0 * rng.standard_normal((nrow, ncol))).astype(np.float32)
    v[rng.random((nrow, ncol)) < 0.1] = np.nan
    return v, NAN


_REF = {}


def reference(shape, name, dtype):
    """the restatement of one zone plane and one value plane, computed once and left unchanged"""
    key = (shape, name, np.dtype(dtype).name)
    if key not in _REF:
        zones, nz = zone_planes(*shape)[name]
        v, nodata = values(*shape, dtype)
        _REF[key] = zr.zonal(v, zones, nodata, n_zones=nz)
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


def _run(hip, stack, zones, **kw):
    import torch
    kw.setdefault("stats", TAB)
    kw.setdefault("planes", ALL)
    table, planes, info = hip.zonal.zonal(stack, torch.from_numpy(np.ascontiguousarray(zones)), **kw)
    return ({k: v.cpu().numpy() for k, v in table.items()} if table is not None else None), {k: v.cpu().numpy() for k, v in planes.items()}, info


def _check(got, want, tag, f32=False, present=False):
    table, planes, info = got
    wtable, wplanes, winfo = want
    if table is not None:
        wt = zr.present(wtable) if present else wtable
        assert list(table) == list(wt), tag
        for k in wt:
            assert _bits(table[k], wt[k]), (tag, "table", k, table[k], wt[k])
    for k in planes:
        w = wplanes[k] if not f32 or wplanes[k].dtype == np.int32 else wplanes[k].astype(np.float32)
        assert _bits(planes[k], w), (tag, "plane", k)
    for k, v in winfo.items():
        assert info[k] == v, (tag, k, info[k], v)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_statistic_on_every_zone_plane_equals_the_restatement(hip, shape):
    import torch
    for dtype in (np.float32, np.int16):
        v, nodata = values(*shape, dtype)
        st = _stack(hip, v[None], nodata)
        for k, (name, (zones, nz)) in enumerate(zone_planes(*shape).items()):
            want = reference(shape, name, dtype)
            tag = (shape, name, np.dtype(dtype).name)
            _check(_run(hip, st, zones, n_zones=nz), want, tag)
            f32 = k % 2 == 0
            _check(_run(hip, st, zones, n_zones=nz, table="present", out_dtype=torch.float32 if f32 else None), want, tag, f32=f32, present=True)
            if dtype == np.float32 and shape[0] * shape[1] > 100:
                assert want[2]["n_inexact"] > 0 or name == "none", tag
    # n_zones measured by the library: max(zone) + 1, which "ends" and "none" put below the number given above
    v, nodata = values(*shape, np.float32)
    st = _stack(hip, v[None], nodata)
    for name in ("own", "ends", "none", "rows"):
        zones, _ = zone_planes(*shape)[name]
        _check(_run(hip, st, zones), zr.zonal(v, zones, nodata), (shape, name, "measured"))
        _check(_run(hip, st, zones, table="present", planes=("dev", "cells")), zr.zonal(v, zones, nodata), (shape, name, "measured"), present=True)


def test_extreme_quanta_exercise_the_high_word_of_s2(hip):
    """+-(2^30 - 1) quanta in every cell of one zone at 67 x 133: the low words of q^2 add up past 2^32 and the high word is in
    use, so the two words must be combined, not carried"""
    rng = np.random.default_rng(3)
    q = np.where(rng.random(BIG) < 0.5, 1, -1) * (2 ** 30 - 1)
    sq = int(q[0, 0]) ** 2
    assert (sq & 0xffffffff) * q.size > 2 ** 32 and sq >> 32 > 0
    v = q.astype(np.float64) * 0.25
    zones = np.zeros(BIG, dtype=np.int32)
    st = _stack(hip, v[None])
    want = zr.zonal(v, zones, n_zones=1, quantum=0.25)
    assert want[2]["n_inexact"] == 0 and want[0]["sd"][0] > 2.0 ** 27
    _check(_run(hip, st, zones, n_zones=1, quantum=0.25), want, "given")
    _check(_run(hip, st, zones), want, "measured")                           # the default quantum is 1/4 here, and n_zones 1
    # the same magnitude everywhere and one sign: sd is exactly 0 out of 120-bit products
    same = np.abs(v)
    got = _run(hip, _stack(hip, same[None]), zones, n_zones=1, quantum=0.25)
    _check(got, zr.zonal(same, zones, n_zones=1, quantum=0.25), "constant")
    assert got[0]["sd"][0] == 0.0 and np.isnan(got[1]["dev"]).all()


def test_nan_inf_and_the_inexact_count(hip):
    rng = np.random.default_rng(5)
    v = (1000.0 + 50.0 * rng.standard_normal(BIG)).astype(np.float32)
    v[3, 5] = np.nan
    v[40, 100] = np.inf
    v[41, 100] = -np.inf
    v[2, 2] = 2.0 ** -20                                                       # far below the quantum: q = 0, inexact
    zones, nz = zone_planes(*BIG)["columns"]
    zones = zones.copy()
    zones[41, 100] = -1                                                        # an Inf without a zone is not counted
    want = zr.zonal(v, zones, n_zones=nz)
    assert want[2]["n_nonfinite"] == 1 and want[2]["n_inexact"] > 0 and want[2]["quantum"] == 2.0 ** -19
    got = _run(hip, _stack(hip, v[None]), zones, n_zones=nz)
    _check(got, want, "nan inf")
    assert np.isnan(got[1]["minus_mean"][40, 100]) and np.isnan(got[1]["minus_mean"][3, 5]) and got[1]["cells"][40, 100] == BIG[0] - 1
    # float64 values, a coarse quantum given: everything is inexact, and the statistics are those of the rounded values
    v64 = v.astype(np.float64)
    want = zr.zonal(v64, zones, n_zones=nz, quantum=4.0)
    assert want[2]["n_inexact"] > BIG[0] * BIG[1] // 2
    _check(_run(hip, _stack(hip, v64[None]), zones, n_zones=nz, quantum=4.0), want, "coarse")


def _dem(hip):
    """a 60 x 80 valley system sloping to a sea of NA cells in the south-east, with voids and a masked lake inland, 30 m cells"""
    r, c = np.meshgrid(np.arange(60.0), np.arange(80.0), indexing="ij")
    rng = np.random.default_rng(31)
    z = 200.0 - 1.5 * r - 1.0 * c + 15.0 * np.sin(c / 6.0) * np.cos(r / 9.0) + rng.standard_normal((60, 80))
    z[r + c > 115] = np.nan
    z[10, 10:13] = np.nan
    z[30:34, 20:25] = np.nan
    z[5, 40] = np.nan
    return z, _stack(hip, z[None].astype(np.float32))


def test_patches_labels_and_flowpath_outlet_labels_as_zones(hip):
    z, st = _dem(hip)
    z32 = st.planes[0].cpu().numpy()
    n = z.size
    # the plateau patches: 8-connected patches of the cells above 120, by label (cell numbers: the present table) and by id
    planes, pinfo = hip.patches.patches(st, 0, "ge", 120.0, 8, ("label", "id"))
    label, ids = planes["label"].cpu().numpy(), planes["id"].cpu().numpy()
    want = zr.zonal(z32, label, n_zones=n)
    table, got_planes, info = hip.zonal.zonal(st, planes["label"], stats=TAB, planes=ALL, n_zones=n, table="present")
    _check(({k: v.cpu().numpy() for k, v in table.items()}, {k: v.cpu().numpy() for k, v in got_planes.items()}, info), want, "label", present=True)
    assert info["n_present"] == pinfo["n_patches"] and table["cells"].sum().item() == pinfo["n_features"]
    zones = ids - 1                                                            # id 1 .. K, 0 off the features
    _check(_run(hip, st, zones), zr.zonal(z32, zones), "id")
    # drainage basins
    hp, _ = hip.hydro(st, 0, ("flowdir",))
    basin, finfo = hip.flowpath.flowpath(hp["flowdir"], st, 0, "outlet", None, "index")
    b = basin.cpu().numpy()
    assert (b >= 0).sum() == finfo["n_valid"] and finfo["n_roots"] > 1
    want = zr.zonal(z32, b, n_zones=n)
    table, got_planes, info = hip.zonal.zonal(st, basin, stats=TAB, planes=ALL, n_zones=n, table="present")
    _check(({k: v.cpu().numpy() for k, v in table.items()}, {k: v.cpu().numpy() for k, v in got_planes.items()}, info), want, "basin", present=True)
    assert info["n_present"] == finfo["n_roots"]


def test_strided_stack_stream_subsets_host_entry_repeat_and_refusals(hip):
    import torch
    from machisplin_amd import _lib
    shape = BIG
    n = shape[0] * shape[1]
    rng = np.random.default_rng(23)
    z = (rng.integers(0, 5000, (3,) + shape) / 4.0).astype(np.float32)
    z[1][rng.random(shape) < 0.05] = np.nan
    st = _stack(hip, z, pad=7)
    zones = (rng.integers(0, 40, shape) * (rng.random(shape) < 0.9) - (rng.random(shape) < 0.05)).astype(np.int32)
    zones[:, 20:60] = 17                                                       # and a coherent band
    want = zr.zonal(z[1], zones, n_zones=40)
    got = _run(hip, st, zones, layer=1, n_zones=40)
    _check(got, want, "padded")
    # the same call made twice gives identical bytes; so does the call without the multi-tile strip
    again = _run(hip, st, zones, layer=1, n_zones=40)
    flat = _run(hip, st, zones, layer=1, n_zones=40, strip=False)
    for other in (again, flat):
        assert all(got[0][k].tobytes() == other[0][k].tobytes() for k in TAB) and all(got[1][k].tobytes() == other[1][k].tobytes() for k in ALL)
        assert got[2] == other[2]
    # given against measured n_zones and quantum: the same bytes where the measured values are the given ones
    given = _run(hip, st, zones, layer=1, n_zones=40, quantum=want[2]["quantum"])
    measured = _run(hip, st, zones, layer=1)
    for other in (given, measured):
        assert all(got[0][k].tobytes() == other[0][k].tobytes() for k in TAB) and all(got[1][k].tobytes() == other[1][k].tobytes() for k in ALL)
    # a non-default stream; int64 zones on the device
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        table, planes, sinfo = hip.zonal.zonal(st, torch.from_numpy(zones).long().cuda(), layer=1, stats=TAB, planes=ALL, n_zones=40, stream=side.cuda_stream)
    side.synchronize()
    _check(({k: v.cpu().numpy() for k, v in table.items()}, {k: v.cpu().numpy() for k, v in planes.items()}, sinfo), want, "stream")
    # subsets, in the caller's order: only what is asked for is made, and a smaller scratch
    sub = _run(hip, st, zones, layer=1, n_zones=40, stats=("max", "count"), planes=("below_max",))
    assert list(sub[0]) == ["max", "count"] and list(sub[1]) == ["below_max"]
    assert _bits(sub[0]["max"], want[0]["max"]) and _bits(sub[0]["count"], want[0]["count"]) and _bits(sub[1]["below_max"], want[1]["below_max"])
    assert sub[2]["scratch_bytes"] < got[2]["scratch_bytes"] <= 40 * 40 + 8 * 6 * 40 + 4 + 256 * 16
    none = _run(hip, st, zones, layer=1, n_zones=40, table=None, planes=("mean",))
    assert none[0] is None and _bits(none[1]["mean"], want[1]["mean"])
    # the host entry against the device entry: a dense table, a present table, planes of both widths
    g = st.geom.c_struct()
    s = _lib.Stack(z.ctypes.data, 3, _lib.F32, n, shape[1], NAN)
    for present in (False, True):
        for f32 in (False, True):
            tab = {k: np.full(40, -7, dtype=np.int64 if k in ("count", "cells") else np.float64) for k in TAB}
            zone = np.full(40, -7, dtype=np.int32)
            pl = {k: np.full(shape, -7, dtype=np.int32 if k in ("count", "cells") else np.float32 if f32 else np.float64) for k in ALL}
            ct = _lib.ZonalTable(40, zone.ctypes.data if present else None, *[tab[k].ctypes.data for k in TAB])
            cp = _lib.ZonalPlanes()
            for k, name in enumerate(ALL):
                cp.plane[k] = pl[name].ctypes.data
            cp.dtype = _lib.F32 if f32 else _lib.F64
            hinfo = _lib.ZonalInfo()
            _lib.check(_lib.lib().mhs_zonal(C.byref(g), C.byref(s), 1, zones.ctypes.data, 40, 0.0, 0, C.byref(ct), C.byref(cp), C.byref(hinfo)))
            k_rows = hinfo.n_present if present else 40
            table = {name: a[:k_rows] for name, a in tab.items()}
            if present:
                table = {"zone": zone[:k_rows], **table}
            _check((table, pl, {name: getattr(hinfo, name) for name, _ in _lib.ZonalInfo._fields_}), want, ("host", present, f32), f32=f32, present=present)
            assert (zone[k_rows:] == -7).all() and all((a[k_rows:] == -7).all() for a in tab.values())
    # the device entry with a row stride of its own on every plane, without info and with both values given: phase 1 is skipped
    wide = torch.full((3, shape[0], shape[1] + 3), 77.0, dtype=torch.float64, device="cuda")
    dtab = torch.full((2, 40), 77.0, dtype=torch.float64, device="cuda")
    zdev = torch.from_numpy(zones).cuda()
    src = st.planes
    cs = _lib.Stack(src.data_ptr(), 3, _lib.F32, src.stride(0), src.stride(1), NAN)

    def direct(n_zones, quantum):
        ct = _lib.ZonalTable(40, None, None, None, dtab[0].data_ptr(), dtab[1].data_ptr())
        cp = _lib.ZonalPlanes()
        for j, k in enumerate((2, 7, 10)):
            cp.plane[k], cp.ld[k] = wide[j].data_ptr(), shape[1] + 3
        cp.dtype = _lib.F64
        rc = _lib.lib().mhs_zonal_dev(C.byref(g), C.byref(cs), 1, zdev.data_ptr(), shape[1], n_zones, quantum, 0, C.byref(ct), C.byref(cp),
                                      torch.cuda.current_stream().cuda_stream, None)
        torch.cuda.synchronize()
        return rc, _lib.lib().mhs_last_error().decode()

    # a zone >= n_zones and a quantum that is too small are refused by name, by the device flag, with nothing written
    for nz, quantum, needle in ((39, want[2]["quantum"], "n_zones"), (40, want[2]["quantum"] / 4, "quantum")):
        rc, msg = direct(nz, quantum)
        assert rc == _lib.ERR_INVALID and needle in msg, msg
        assert (wide == 77.0).all().item() and (dtab == 77.0).all().item()
    rc, msg = direct(40, want[2]["quantum"])
    assert rc == _lib.OK, msg
    w = wide.cpu().numpy()
    for j, name in enumerate(("mean", "minus_mean", "dev")):
        assert _bits(np.ascontiguousarray(w[j, :, :shape[1]]), want[1][name]), name
    assert (w[:, :, shape[1]:] == 77.0).all()
    assert _bits(dtab[0].cpu().numpy(), want[0]["mean"]) and _bits(dtab[1].cpu().numpy(), want[0]["sd"])
    # the same refusals where phase 1 runs (info is asked for): found before any table is written
    with pytest.raises(hip.MhsError, match="n_zones"):
        _run(hip, st, zones, layer=1, n_zones=39)
    with pytest.raises(hip.MhsError, match="quantum"):
        _run(hip, st, zones, layer=1, n_zones=40, quantum=want[2]["quantum"] / 4)


def test_mid_size_plane_with_a_few_thousand_coherent_zones(hip):
    """1 500 x 1 700 cells in blocks of 30 x 31 with ragged edges: 50 x 55 zones.  The values are whole numbers below 2^15, so
    S2 < 2^63 and np.add.at on int64 is an exact reference of its own, beside the restatement"""
    import torch
    shape = (1500, 1700)
    rng = np.random.default_rng(41)
    r, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    shift = rng.integers(-3, 4, shape[0])[:, None]
    zones = ((r // 30) * 55 + np.clip(c + shift, 0, shape[1] - 1) // 31).astype(np.int32)
    zones[rng.random(shape) < 0.01] = -1
    nz = int(zones.max()) + 1
    v = rng.integers(-2000, 30000, shape).astype(np.float32)
    v[rng.random(shape) < 0.02] = np.nan
    ok = (zones >= 0) & ~np.isnan(v)
    q = v[ok].astype(np.int64)
    S1 = np.zeros(nz, dtype=np.int64)
    S2 = np.zeros(nz, dtype=np.int64)
    np.add.at(S1, zones[ok], q)
    np.add.at(S2, zones[ok], q * q)
    cnt = np.bincount(zones[ok], minlength=nz)
    st = _stack(hip, v[None])
    table, planes, info = hip.zonal.zonal(st, torch.from_numpy(zones), stats=TAB, planes=("mean", "minus_mean", "dev", "count"), n_zones=nz, quantum=1.0,
                                          out_dtype=torch.float32)
    table = {k: a.cpu().numpy() for k, a in table.items()}
    planes = {k: a.cpu().numpy() for k, a in planes.items()}
    assert info["n_inexact"] == 0 and info["n_contributing"] == ok.sum() and 2500 < info["n_present"] <= nz
    assert np.array_equal(table["count"], cnt) and _bits(table["sum"], S1.astype(np.float64)) and _bits(table["mean"], S1.astype(np.float64) / cnt)
    num = np.array([int(n) * int(b) - int(a) * int(a) for n, a, b in zip(cnt, S1, S2)], dtype=object)
    sd = np.array([np.sqrt(float(x) / (float(n) * float(n - 1))) for x, n in zip(num, cnt)])             # num < 2^64 here: D(x) = (double)x
    assert max(int(x) for x in num) < 2 ** 64 and _bits(table["sd"], sd)
    want = zr.zonal(v, zones, n_zones=nz, quantum=1.0)
    _check((table, planes, info), want, "mid", f32=True)


def test_covariates_basin_specs(hip):
    import torch
    from machisplin_amd import terrain
    z, st = _dem(hip)
    old = ("slope_deg", "twi", ("hand", 50), "flowdist_outlet", "dist_na")
    cov = terrain.covariates(st, old + ("basin_mean", "basin_minus_mean", "basin_dev"))
    assert cov.names == ["dem", "slope_deg", "twi", "hand50", "flowdist_outlet", "dist_na", "basin_mean", "basin_minus_mean", "basin_dev"]
    assert cov.planes.dtype == torch.float32
    # an old spec list gives unchanged bytes with and without the new specs beside it
    plain = terrain.covariates(st, old)
    assert plain.planes.cpu().numpy().tobytes() == cov.planes[:6].cpu().numpy().tobytes()
    one = terrain.covariates(st, ("basin_dev", "twi"))
    assert one.names == ["dem", "basin_dev", "twi"] and torch.equal(one.planes[1].view(torch.int32), cov.planes[8].view(torch.int32))
    assert torch.equal(one.planes[2].view(torch.int32), cov.planes[2].view(torch.int32))
    # against flowpath + the restatement
    hp, _ = hip.hydro(st, 0, ("flowdir",))
    basin = hip.flowpath.flowpath(hp["flowdir"], st, 0, "outlet", None, "index")[0].cpu().numpy()
    _, want, _ = zr.zonal(st.planes[0].cpu().numpy(), basin, n_zones=z.size, f32=True)
    for k, name in ((6, "mean"), (7, "minus_mean"), (8, "dev")):
        assert _bits(cov.planes[k].cpu().numpy(), want[name]), name
    assert np.isnan(want["mean"][np.isnan(z)]).all() and np.isfinite(want["dev"]).sum() > z.size // 4
    for bad in (("basin_mean", 3), ("basin_dev", 1, 2)):
        with pytest.raises(ValueError, match=bad[0]):
            terrain.covariates(st, (bad,))
