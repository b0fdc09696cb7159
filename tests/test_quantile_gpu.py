"""GPU: zonal quantiles (include/machisplin_hip.h, section "zonal quantiles"; csrc/quantile.hip on csrc/sort_keys.hip).  Every
table, plane and info field equals the numpy restatement of tests/quantile_ref.py BIT FOR BIT (the bytes are compared, NaN
included).

Shapes: the degenerate ones, every combination of one less than, exactly and one more than a tile of "zonal" in the two
dimensions (ZONAL_TILE_ROWS, ZONAL_TILE_COLS, read from the text of csrc/zonal_rule.h), and one whose cell count is just past two
tiles of the sort (SORT_TILE_KEYS of csrc/sort_keys.h).  Each is crossed with the zone planes that stress the sort and the
segment search: one zone (one long segment), every cell its own zone (segments of one), pairs, one-column and one-row stripes, a
checkerboard, no zone at all, and a zone that occurs at the two ends of the plane only."""
import os
import re

import numpy as np
import pytest

import quantile_ref as qr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
PLANES = ("q", "below", "frac_below")
P1, P7 = (0.5,), (0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 1.0, 0.5)


def _constant(name, header="zonal_rule.h"):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def _define(name):
    text = open(os.path.join(ROOT, "include", "machisplin_hip.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


TR, TC, T = _constant("ZONAL_TILE_ROWS"), _constant("ZONAL_TILE_COLS"), _constant("SORT_TILE_KEYS", "sort_keys.h")
TILE_BYTES, FIXED = _constant("SORT_TILE_BYTES", "sort_keys.h"), _define("MHS_QUANTILE_SCRATCH_FIXED")
PAST_2T = (2 * T // 61 + 1, 61)                                                # 68 x 61 = 4 148 cells at T = 2 048: the third tile holds 52
SHAPES = [(1, 1), (1, TC + 1), (TR + 1, 1)] + [(r, c) for r in (TR - 1, TR, TR + 1) for c in (TC - 1, TC, TC + 1)] + [PAST_2T]
assert 2 * T < PAST_2T[0] * PAST_2T[1] < 2 * T + 64


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
    """(plane, nodata): random values with ~10 % NA; the float32 ones are not multiples of the default quantum"""
    rng = np.random.default_rng(nrow * 1000 + ncol)
    if dtype == np.int16:
        v = rng.integers(-500, 9000, (nrow, ncol)).astype(np.int16)
        v[rng.random((nrow, ncol)) < 0.1] = -32768
        return v, -32768.0
    v = (100.0 * rng.standard_normal((nrow, ncol))).astype(np.float32)
    v[rng.random((nrow, ncol)) < 0.1] = np.nan
    return v, NAN


_REF = {}


def reference(shape, name, dtype, probs):
    """the restatement of one zone plane and one value plane, computed once and left unchanged"""
    key = (shape, name, np.dtype(dtype).name, probs)
    if key not in _REF:
        zones, nz = zone_planes(*shape)[name]
        v, nodata = values(*shape, dtype)
        _REF[key] = qr.quantile(v, zones, probs, nodata, n_zones=nz)
    return _REF[key]


def _stack(hip, layers, nodata=NAN, pad=0, geom=None):
    """a RasterStack; pad > 0: cut out of a tensor with `pad` more columns and one more layer"""
    import torch
    layers = np.asarray(layers)
    n, nr, nc = layers.shape
    st = hip.RasterStack(geom or hip.Geometry(1000.0, 5000.0, 30.0, 30.0, nr, nc), layers, nodata)
    if pad:
        big = torch.full((n + 1, nr, nc + pad), 5, dtype=st.planes.dtype, device=st.planes.device)
        big[1:, :, :nc] = st.planes
        st.planes = big[1:, :, :nc]
        assert st.planes.stride(1) == nc + pad
    return st


def _run(hip, stack, zones, **kw):
    import torch
    kw.setdefault("planes", PLANES)
    z = torch.from_numpy(np.ascontiguousarray(zones)) if zones is not None else None
    table, planes, info = hip.zonal.quantile(stack, z, **kw)
    return ({k: v.cpu().numpy() for k, v in table.items()} if table is not None else None), {k: v.cpu().numpy() for k, v in planes.items()}, info


def _check(got, want, tag, f32=False, present=False):
    table, planes, info = got
    wtable, wplanes, winfo = want
    if table is not None:
        wt = qr.present(wtable) if present else wtable
        assert sorted(table) == sorted(wt), tag
        for k in wt:
            assert _bits(table[k], wt[k]), (tag, "table", k, table[k], wt[k])
    for k in planes:
        w = wplanes[k] if not f32 or wplanes[k].dtype == np.int32 else wplanes[k].astype(np.float32)
        assert _bits(planes[k], w), (tag, "plane", k)
    for k, v in winfo.items():
        assert info[k] == v, (tag, k, info[k], v)
    assert 0 <= info["passes_run"] <= 8, tag


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_product_on_every_zone_plane_equals_the_restatement(hip, shape):
    import torch
    for dtype in (np.float32, np.int16):
        v, nodata = values(*shape, dtype)
        st = _stack(hip, v[None], nodata)
        for k, (name, (zones, nz)) in enumerate(zone_planes(*shape).items()):
            probs = P7 if k % 2 == 0 else P1
            want = reference(shape, name, dtype, probs)
            tag = (shape, name, np.dtype(dtype).name)
            _check(_run(hip, st, zones, probs=probs, n_zones=nz), want, tag)
            f32 = k % 4 < 2
            _check(_run(hip, st, zones, probs=probs, n_zones=nz, table="present", out_dtype=torch.float32 if f32 else None), want, tag, f32=f32,
                   present=True)
            if dtype == np.float32 and shape[0] * shape[1] > 100:
                assert want[2]["n_inexact"] > 0 or name == "none", tag
    # n_zones measured by the library: max(zone) + 1, which "ends" and "none" put below the number given above
    v, nodata = values(*shape, np.float32)
    st = _stack(hip, v[None], nodata)
    for name in ("own", "ends", "none", "rows"):
        zones, _ = zone_planes(*shape)[name]
        want = qr.quantile(v, zones, P7, nodata)
        _check(_run(hip, st, zones, probs=P7), want, (shape, name, "measured"))
        _check(_run(hip, st, zones, probs=P7, table="present", planes=("frac_below",)), want, (shape, name, "measured"), present=True)
        _check(_run(hip, st, zones, probs=P7, table=None, planes=("q",)), want, (shape, name, "planes only"))


def test_present_form_on_huge_zone_numbers_allocates_nothing_by_n_zones(hip):
    """zones 0, 2^24 + 3 and 2^31 - 2 with n_zones = 2^31 - 1 on 9 x 70 cells: the present table is right and the scratch is that
    of the cells -- 16 bytes each, the tiles' blocks and the header's fixed part; a dense table of 2^31 - 1 rows would be 16 GB"""
    shape = (9, 70)
    rng = np.random.default_rng(5)
    v, nodata = values(*shape, np.float32)
    names = np.array([0, 2 ** 24 + 3, 2 ** 31 - 2, -1], dtype=np.int64)
    zones = names[rng.integers(0, 4, shape)].astype(np.int32)
    st = _stack(hip, v[None], nodata)
    table, _, info = _run(hip, st, zones, probs=P7, n_zones=2 ** 31 - 1, table="present", planes=())
    # the restatement on the renumbered zones 0, 1, 2
    small = np.searchsorted(names[:3], np.where(zones < 0, 0, zones)).astype(np.int32)
    small[zones < 0] = -1
    wt, _, winfo = qr.quantile(v, small, P7, nodata, n_zones=3)
    assert table["zone"].tolist() == [0, 2 ** 24 + 3, 2 ** 31 - 2]
    assert _bits(table["q"], wt["q"]) and _bits(table["count"], wt["count"])
    for k in ("n_present", "n_cells_in_zones", "n_contributing", "n_inexact", "quantum"):
        assert info[k] == winfo[k], k
    ncell = shape[0] * shape[1]
    tiles = -(-ncell // T)
    assert info["n_zones"] == 2 ** 31 - 1 and info["scratch_bytes"] <= 16 * ncell + (TILE_BYTES + 4) * tiles + FIXED, info
    assert info["passes_run"] == 8                                             # the zone numbers reach into every byte above the values'


def test_p0_p1_and_count_equal_zonal_on_the_device(hip):
    import torch
    shape = (TR + 1, TC + 1)
    for dtype in (np.float32, np.int16):
        v, nodata = values(*shape, dtype)
        st = _stack(hip, v[None], nodata)
        for name in ("pairs", "columns", "ends", "one"):
            zones, nz = zone_planes(*shape)[name]
            z = torch.from_numpy(zones)
            zt, _, zinfo = hip.zonal.zonal(st, z, stats=("min", "max", "count"), n_zones=nz)
            qt, _, qinfo = hip.zonal.quantile(st, z, probs=(0.0, 1.0), n_zones=nz)
            assert torch.equal(qt["q"][:, 0].view(torch.int64), zt["min"].view(torch.int64)), (name, dtype)
            assert torch.equal(qt["q"][:, 1].view(torch.int64), zt["max"].view(torch.int64)), (name, dtype)
            assert torch.equal(qt["count"], zt["count"]), (name, dtype)
            for k in ("n_zones", "n_cells_in_zones", "n_contributing", "n_nonfinite", "n_inexact", "quantum"):
                assert qinfo[k] == zinfo[k], (name, k)


def test_aggregate_quantile_equals_resample_min_max_count_and_the_restatement(hip):
    """a target that does not divide the source and is shifted by a fraction of a cell, reaching past the source: target cells
    with an empty footprint hold NaN and count 0"""
    from machisplin_amd import resample
    X0, Y0, DX, DY = 1000.0, 5000.0, 30.0, 30.0
    shape = (TR + 9, 2 * TC + 5)
    S = hip.Geometry(X0, Y0, DX, DY, *shape)
    targets = (hip.Geometry(X0 + 1.3 * DX, Y0 - 0.7 * DY, 3.7 * DX, 3.7 * DY, int(shape[0] / 3.7) + 3, int(shape[1] / 3.7) + 3),
               hip.Geometry(X0 - 2.25 * DX, Y0 + 1.5 * DY, 11.0 * DX, 6.5 * DY, 6, 14))
    probs = (0.0, 1.0, 0.5, 0.9)
    for dtype in (np.float32, np.int16):
        v, nodata = values(*shape, dtype)
        if dtype == np.float32:
            v = (np.rint(v * 16.0) / 16.0).astype(np.float32)                 # exact at the default quantum: min and max are the values' own
        st = _stack(hip, v[None], nodata, geom=S)
        for Tg in targets:
            q, count, info = hip.zonal.aggregate_quantile(st, Tg, probs=probs)
            wq, wcount, winfo = qr.aggregate_quantile(v, S, Tg, probs, nodata)
            assert winfo["n_inexact"] == 0 and (wcount == 0).any() and (wcount > 1).any()
            assert _bits(q.cpu().numpy(), wq) and _bits(count.cpu().numpy(), wcount)
            for k, w in winfo.items():
                assert info[k] == w, (k, info[k], w)
            import torch
            for j, method in ((0, "min"), (1, "max")):
                r = resample.resample(st, Tg, method, out_dtype=torch.float64).planes[0]
                assert _bits(q[j].cpu().numpy(), r.cpu().numpy()), (method, dtype)
            r = resample.resample(st, Tg, "count", out_dtype=torch.float64).planes[0]
            assert np.array_equal(r.cpu().numpy(), count.cpu().numpy().astype(np.float64))
        q32, _, _ = hip.zonal.aggregate_quantile(st, targets[0], probs=probs, out_dtype=torch.float32)
        assert _bits(q32.cpu().numpy(), qr.aggregate_quantile(v, S, targets[0], probs, nodata)[0].astype(np.float32))


def test_whole_layer_form_equals_numpy_quantile_of_the_quantised_values(hip):
    shape = PAST_2T
    for dtype in (np.float32, np.int16):
        v, nodata = values(*shape, dtype)
        st = _stack(hip, v[None], nodata)
        got = _run(hip, st, None, probs=P7)
        want = qr.quantile(v, None, P7, nodata)
        _check(got, want, ("whole", dtype))
        _check(_run(hip, st, None, probs=P7, table="present"), want, ("whole", dtype), present=True)
        # the rule's value against numpy's on the quantised values: within twice the header's bound; the median bit for bit
        x = v.astype(np.float64)
        ok = ~np.isnan(x) & (x != nodata)
        quantum = got[2]["quantum"]
        s = np.sort(np.rint(x[ok] / quantum).astype(np.int64))
        b = qr.bound(s, quantum)
        for j, p in enumerate(P7):
            assert abs(got[0]["q"][0, j] - float(np.quantile(s.astype(np.float64) * quantum, p, method="linear"))) <= 2 * b, (dtype, p)
        assert got[0]["q"][0, 3] == float(np.median(s.astype(np.float64) * quantum)) and got[0]["count"][0] == s.size


def test_a_strided_stack_a_second_layer_and_a_repeat(hip):
    shape = (TR + 1, TC + 1)
    v, nodata = values(*shape, np.float32)
    other = np.zeros(shape, dtype=np.float32)
    zones, nz = zone_planes(*shape)["pairs"]
    want = qr.quantile(v, zones, P7, nodata, n_zones=nz)
    st = _stack(hip, np.stack([other, v]), nodata, pad=7)
    a = _run(hip, st, zones, probs=P7, n_zones=nz, layer=1)
    _check(a, want, "strided")
    b = _run(hip, st, zones, probs=P7, n_zones=nz, layer=1)
    for k in a[1]:
        assert a[1][k].tobytes() == b[1][k].tobytes()
    assert a[0]["q"].tobytes() == b[0]["q"].tobytes()
    # a zone plane with a row stride of its own and int64 zones
    import torch
    wide = torch.full((shape[0], shape[1] + 3), 10 ** 6, dtype=torch.int32, device="cuda")
    wide[:, :shape[1]] = torch.from_numpy(zones).cuda()
    table, planes, info = hip.zonal.quantile(st, wide[:, :shape[1]], probs=P7, n_zones=nz, layer=1, planes=PLANES)
    _check(({k: t.cpu().numpy() for k, t in table.items()}, {k: t.cpu().numpy() for k, t in planes.items()}, info), want, "strided zones")


def test_a_zone_beyond_n_zones_is_refused_with_nothing_written(hip, monkeypatch):
    import torch
    from machisplin_amd import _lib
    shape = (TR + 1, TC + 1)
    v, nodata = values(*shape, np.float32)
    zones, nz = zone_planes(*shape)["columns"]
    st = _stack(hip, v[None], nodata)
    marker = 12345.0
    made = []
    real_empty = torch.empty

    def marked(*a, **kw):                                                      # every output tensor is pre-filled with the marker
        t = real_empty(*a, **kw)
        t.fill_(marker if t.dtype.is_floating_point else 12345)
        made.append(t)
        return t

    monkeypatch.setattr(torch, "empty", marked)
    with pytest.raises(_lib.MhsError, match="n_zones"):
        hip.zonal.quantile(st, torch.from_numpy(zones), probs=P7, n_zones=nz - 1, planes=PLANES)
    with pytest.raises(_lib.MhsError, match="n_zones"):
        hip.zonal.quantile(st, torch.from_numpy(zones), probs=P7, n_zones=nz - 1, table="present", planes=PLANES)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(made) >= 8
    for t in made:
        assert bool((t == (marker if t.dtype.is_floating_point else 12345)).all()), (t.dtype, t.shape)


def test_host_entry_equals_the_device_entry(hip):
    import ctypes as C
    from machisplin_amd import _lib
    shape = (TR + 1, TC + 1)
    v, nodata = values(*shape, np.float32)
    zones, nz = zone_planes(*shape)["pairs"]
    want = qr.quantile(v, zones, P7, nodata, n_zones=nz, f32=True)
    n = shape[0] * shape[1]
    q = np.full((nz, len(P7)), 7.0)
    count = np.full(nz, 7, dtype=np.int64)
    zone = np.full(nz, 7, dtype=np.int32)
    qp = np.full((len(P7),) + shape, 7.0, dtype=np.float32)
    below = np.full(shape, 7, dtype=np.int32)
    frac = np.full(shape, 7.0, dtype=np.float32)
    g = _lib.Grid(1000.0, 5000.0, 30.0, 30.0, *shape)
    stack = _lib.Stack(v.ctypes.data, 1, _lib.F32, n, shape[1], NAN)
    pl = _lib.QuantilePlanes()
    for j in range(len(P7)):
        pl.q[j] = qp[j].ctypes.data
    pl.below, pl.frac_below, pl.dtype = below.ctypes.data, frac.ctypes.data, _lib.F32
    probs = (C.c_double * len(P7))(*P7)
    info = _lib.QuantileInfo()
    for present in (False, True):
        tab = _lib.QuantileTable(nz, zone.ctypes.data if present else None, count.ctypes.data, q.ctypes.data)
        _lib.check(_lib.lib().mhs_zonal_quantile(C.byref(g), C.byref(stack), 0, zones.ctypes.data, nz, 0.0, 0, probs, len(P7), None, C.byref(tab),
                                                 C.byref(pl), C.byref(info)))
        wt = qr.present(want[0]) if present else want[0]
        k = wt["count"].size
        assert _bits(q[:k], wt["q"]) and _bits(count[:k], wt["count"]) and (not present or _bits(zone[:k], wt["zone"]))
        assert _bits(qp, want[1]["q"]) and _bits(below, want[1]["below"]) and _bits(frac, want[1]["frac_below"])
        assert info.n_present == want[2]["n_present"] and info.n_contributing == want[2]["n_contributing"] and info.quantum == want[2]["quantum"]
    # the whole layer and a target through the host entry
    S = hip.Geometry(1000.0, 5000.0, 30.0, 30.0, *shape)
    Tg = hip.Geometry(1040.0, 4980.0, 111.0, 111.0, 9, 19)
    tg = Tg.c_struct()
    cap = Tg.nrow * Tg.ncol
    q2, c2 = np.zeros((cap, len(P7))), np.zeros(cap, dtype=np.int64)
    tab = _lib.QuantileTable(cap, None, c2.ctypes.data, q2.ctypes.data)
    _lib.check(_lib.lib().mhs_zonal_quantile(C.byref(g), C.byref(stack), 0, None, 0, 0.0, 0, probs, len(P7), C.byref(tg), C.byref(tab), None, None))
    wq, wc, _ = qr.aggregate_quantile(v, S, Tg, P7, nodata)
    assert _bits(q2.T.reshape(wq.shape).copy(), wq) and _bits(c2.reshape(wc.shape), wc)


def test_covariates_with_the_four_quantile_specs(hip):
    """basin_median / basin_frac_below against hydro_ref -> flowpath_ref -> the restatement, zone_median / zone_frac_below against
    rasterize_ref -> the restatement; an old spec list gives the same bytes with and without the new specs beside it"""
    import torch

    import flowpath_ref as fr
    import hydro_ref as hr
    import rasterize_ref as rr
    from machisplin_amd import terrain
    from machisplin_amd.vector import Features
    g = hip.Geometry(1000.0, 5000.0, 30.0, 30.0, 60, 80)
    r, c = np.meshgrid(np.arange(60.0), np.arange(80.0), indexing="ij")
    z = 200.0 - 1.5 * r - 1.0 * c + 15.0 * np.sin(c / 6.0) * np.cos(r / 9.0) + np.random.default_rng(31).standard_normal((60, 80))
    z[r + c > 115] = np.nan
    z[30:34, 20:25] = np.nan
    z = z.astype(np.float32)
    st = hip.RasterStack(g, torch.from_numpy(z[None]).cuda(), NAN)
    units = Features.from_parts("polygon", [[ring] for ring in rr.lattice(g, 4, 5, 2, zigzag=3)][:-3])    # the last three units are missing
    old = ("slope_deg", "twi", "basin_mean", ("zone_dev", units))
    new = ("basin_median", "basin_frac_below", ("zone_median", units), ("zone_frac_below", units))
    cov = terrain.covariates(st, old + new)
    assert cov.names == ["dem", "slope_deg", "twi", "basin_mean", "zone_dev", "basin_median", "basin_frac_below", "zone_median", "zone_frac_below"]
    assert cov.planes.dtype == torch.float32
    plain = terrain.covariates(st, old)
    assert plain.planes.cpu().numpy().tobytes() == cov.planes[:5].cpu().numpy().tobytes()
    # the old names against direct zonal calls on the library's own zone planes
    hp, _ = hip.hydro(st, 0, ("flowdir",))
    basin_dev = hip.flowpath.flowpath(hp["flowdir"], st, 0, "outlet", None, "index")[0]
    direct = hip.zonal.zonal(st, basin_dev, 0, stats=(), planes=("mean",), n_zones=z.size, table=None, out_dtype=torch.float32)[1]["mean"]
    assert torch.equal(direct.view(torch.int32), plain.planes[3].view(torch.int32))
    only_new = terrain.covariates(st, new[1:2] + new[2:3])
    assert only_new.names == ["dem", "basin_frac_below", "zone_median"]
    assert torch.equal(only_new.planes[1].view(torch.int32), cov.planes[6].view(torch.int32))
    assert torch.equal(only_new.planes[2].view(torch.int32), cov.planes[7].view(torch.int32))
    # the restatement, composed
    flowdir = hr.hydro(z, NAN, 30.0, 30.0)["flowdir"]
    basin = fr.flowpath(flowdir, z, NAN, "outlet")[0]["index"]
    assert np.array_equal(basin, basin_dev.cpu().numpy())
    _, wb, _ = qr.quantile(z, basin, (0.5,), n_zones=z.size, f32=True)
    zone = rr.rasterize(units, g)[0]["index"]
    _, wz, _ = qr.quantile(z, zone, (0.5,), n_zones=len(units), f32=True)
    got = cov.planes.cpu().numpy()
    assert _bits(got[5], wb["q"][0]) and _bits(got[6], wb["frac_below"]) and _bits(got[7], wz["q"][0]) and _bits(got[8], wz["frac_below"])
    assert np.isnan(got[5][np.isnan(z)]).all() and np.isnan(got[7][zone < 0]).all() and (zone < 0).sum() > 100
    inside = ~np.isnan(got[6])
    assert inside.sum() > z.size // 2 and (got[6][inside] >= 0).all() and (got[6][inside] < 1).all()
    for bad in (("basin_median", 3), ("zone_median",), ("zone_frac_below", units, 1), ("zone_median", 3)):
        with pytest.raises(ValueError, match=bad[0]):
            terrain.covariates(st, (bad,))
