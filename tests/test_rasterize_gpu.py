"""GPU: rasterize on the device (csrc/rasterize.hip) equals the numpy restatement of the rule (tests/rasterize_ref.py) exactly,
in every plane and in every field of the info that does not describe the scratch plan.  The grid shapes are the word and wave
boundaries of the bit plane (32 columns to a word, RZ_CHUNK_WORDS words to a wave's chunk), the vertex counts pass the block
of the edge prefix sum (RZ_SCAN_BLOCK), and the scratch budgets force 1, 3 and n batches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rasterize_ref as rr
import zonal_ref as zr
from machisplin_amd import Geometry, _lib
from machisplin_amd.vector import Features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_H = open(os.path.join(ROOT, "machisplin_amd", "csrc", "rasterize_rule.h")).read()
SCAN_BLOCK = int(re.search(r"RZ_SCAN_BLOCK = (\d+)", RULE_H).group(1))
CHUNK_COLS = 32 * int(re.search(r"RZ_CHUNK_WORDS = (\d+)", RULE_H).group(1))
ALL = ("index", "count", "value")
NP = {None: np.float64, "f64": np.float64, "f32": np.float32}


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def grid(nrow, ncol, xres=1.5, yres=2.0):
    return Geometry(100.0, 900.0, xres, yres, nrow, ncol)


def on_grid(g, u, v):
    """grid fractions (u to the east, v to the south; 0 .. 1 is the extent) as coordinates"""
    return np.column_stack([g.xmin + np.asarray(u) * g.ncol * g.xres, g.ymax - np.asarray(v) * g.nrow * g.yres])


def star(g, u, v, r_in, r_out, n, seed):
    s = rr.star(u, v, r_in, r_out, n, seed)
    return on_grid(g, s[:, 0], s[:, 1])


def scene(g, seed=0):
    """overlapping polygons all over the grid and beyond it: a star with a hole, a two-part feature, a feature whose hole touches
    nothing of it (an island under even-odd), triangles that leave the grid on each side and at each corner, with tied values"""
    rng = np.random.default_rng(seed)
    feats = [[star(g, 0.45, 0.5, 0.25, 0.45, 40, seed), star(g, 0.45, 0.5, 0.05, 0.2, 8, seed + 1)],
             [star(g, 0.2, 0.25, 0.05, 0.2, 9, seed + 2), star(g, 0.8, 0.7, 0.05, 0.25, 11, seed + 3)],
             [star(g, 0.7, 0.3, 0.1, 0.2, 7, seed + 4), star(g, 0.15, 0.8, 0.03, 0.1, 5, seed + 5)]]
    for u, v in ((-0.1, 0.5), (1.1, 0.5), (0.5, -0.1), (0.5, 1.1), (-0.05, -0.05), (1.05, -0.05), (-0.05, 1.05), (1.05, 1.05)):
        feats.append([star(g, u, v, 0.1, 0.3, 3, int(rng.integers(1000)))])
    values = np.array([3.0, 1.5, 3.0, -2.0, 1.5, 7.25, 0.0, 3.0, -2.0, 1.5, 9.0])
    return Features.from_parts("polygon", feats, values)


def run(hip, ft, g, rule="last", touches=False, products=ALL, dtype=None, want=None, **kw):
    """one device call against the restatement: every plane's bytes, every field of rr.INFO"""
    import torch
    from machisplin_amd.rasterize import rasterize
    if want is None:
        want = rr.rasterize(ft, g, rule, touches, NP[dtype])
    planes, info = rasterize(ft, g, products, rule, touches, {None: None, "f64": torch.float64, "f32": torch.float32}[dtype], **kw)
    torch.cuda.synchronize()
    assert tuple(planes) == tuple(products)
    for p in products:
        got = planes[p].cpu().numpy()
        assert bits_equal(got, want[0][p]), (p, rule, touches, int((got != want[0][p]).sum()), np.argwhere(got != want[0][p])[:5].tolist())
    assert {k: info[k] for k in rr.INFO} == want[1], (info, want[1])
    return planes, info


SHAPES = [(1, 1), (1, 65), (33, 1)] + [(r, c) for r in (31, 32, 33) for c in (63, 64, 65)] + [(67, 133)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_shapes_at_the_word_and_wave_boundaries(hip, shape):
    g = grid(*shape)
    ft = scene(g, 3)
    run(hip, ft, g, "last", False)
    run(hip, ft, g, "max", True, dtype="f32")
    run(hip, ft.rings_as_lines(), g, "first")
    rng = np.random.default_rng(5)
    pts = on_grid(g, rng.uniform(-0.1, 1.1, 300), rng.uniform(-0.1, 1.1, 300))
    run(hip, Features("point", pts, np.arange(301), np.arange(301), rng.integers(0, 5, 300).astype(float)), g, "min")


@pytest.mark.parametrize("shape", [(3, 2100), (2, 4100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wide_boxes_cross_the_chunk_carry_of_the_fill_scan(hip, shape):
    g = grid(*shape, xres=1.0, yres=1.0)
    assert g.ncol > CHUNK_COLS and (shape[1] < 2 * CHUNK_COLS) == (shape[1] == 2100)
    rng = np.random.default_rng(shape[1])
    # a comb over the full width: teeth of odd widths, so that a row's crossings fall in every chunk and change the carried parity
    u = np.sort(rng.uniform(0.0, 1.0, 90))
    top = np.column_stack([u, np.where(np.arange(90) % 2, -0.2, rng.uniform(0.2, 0.9, 90))])
    ring = np.vstack([[-0.01, 1.2], top, [1.01, 1.2], [-0.01, 1.2]])
    inner = np.array([[0.3, 0.1], [0.97, 0.1], [0.97, 0.8], [0.3, 0.8], [0.3, 0.1]])
    ft = Features.from_parts("polygon", [[on_grid(g, ring[:, 0], ring[:, 1])], [on_grid(g, inner[:, 0], inner[:, 1])]], [1.0, 2.0])
    for touches in (False, True):
        run(hip, ft, g, "last", touches)
    run(hip, ft.rings_as_lines(), g, "first")


def test_many_edges_pass_the_blocks_of_the_prefix_sum(hip):
    g = grid(150, 170)
    n = 5000
    assert n > 2 * SCAN_BLOCK
    rng = np.random.default_rng(8)
    v = np.sort(rng.uniform(0.02, 0.98, n - 2))
    u = 0.7 + 0.25 * np.sin(40.0 * v) * rng.uniform(0.2, 1.0, n - 2)
    # one edge 150 rows tall from the south-west to the north-west, then 4 999 short ones back down a ragged east side
    ring = np.vstack([[0.1, 1.05], [0.12, -0.05], np.column_stack([u, v]), [0.1, 1.05]])
    assert ring.shape[0] == n + 1
    ft = Features.from_parts("polygon", [[on_grid(g, ring[:, 0], ring[:, 1])], [star(g, 0.4, 0.5, 0.1, 0.3, 2100, 1)]], [1.0, 2.0])
    _, info = run(hip, ft, g, "last", False)
    assert info["n_edges"] == n + 2100
    run(hip, ft, g, "first", True)


def test_polygon_cases(hip):
    g = grid(67, 133)
    sq = lambda u0, v0, u1, v1: on_grid(g, [u0, u1, u1, u0, u0], [v0, v0, v1, v1, v0])      # noqa: E731
    cases = {
        "wholly outside": [[sq(1.2, 0.2, 1.6, 0.6)], [sq(-0.5, -0.5, -0.1, -0.1)], [sq(0.2, 1.01, 0.6, 1.3)], [sq(0.2, -3.0, 0.6, -0.001)]],
        "contains the grid": [[sq(-0.5, -0.5, 1.5, 1.5)]],
        "exactly the extent": [[sq(0.0, 0.0, 1.0, 1.0)]],
        "each side and corner": [[sq(-0.2, 0.3, 0.2, 0.6)], [sq(0.8, 0.3, 1.2, 0.6)], [sq(0.3, -0.2, 0.6, 0.2)], [sq(0.3, 0.8, 0.6, 1.2)],
                                 [sq(-0.2, -0.2, 0.1, 0.1)], [sq(0.9, -0.2, 1.2, 0.1)], [sq(-0.2, 0.9, 0.1, 1.2)], [sq(0.9, 0.9, 1.2, 1.2)]],
        "holes and an island": [[sq(0.1, 0.1, 0.9, 0.9), sq(0.2, 0.2, 0.4, 0.4), sq(0.5, 0.5, 0.8, 0.8), sq(0.6, 0.6, 0.7, 0.7)],
                                [sq(0.05, 0.05, 0.3, 0.3), sq(0.93, 0.93, 0.99, 0.99)]],
        "self-overlapping": [[on_grid(g, [0.1, 0.9, 0.1, 0.9, 0.1], [0.1, 0.9, 0.9, 0.1, 0.1])],                                  # a bow tie
                             [on_grid(g, 0.5 + 0.4 * np.sin(np.arange(6) * 0.8 * np.pi), 0.5 - 0.4 * np.cos(np.arange(6) * 0.8 * np.pi))]],
        "zero area": [[on_grid(g, [0.2, 0.8, 0.8, 0.2], [0.3, 0.6, 0.6, 0.3])], [on_grid(g, [0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5])],
                      [sq(0.3, 0.5, 0.7, 0.5)]],
        "on cell centres": [[on_grid(g, (np.array([10, 40, 40, 10, 10]) + 0.5) / 133, (np.array([5, 5, 30, 30, 5]) + 0.5) / 67)]],
    }
    pentagram = cases["self-overlapping"][1][0]
    pentagram[-1] = pentagram[0]                                                # closed exactly
    for name, feats in cases.items():
        ft = Features.from_parts("polygon", feats, np.arange(len(feats), dtype=float))
        for touches in (False, True):
            _, info = run(hip, ft, g, "last", touches)
            if name == "wholly outside":
                assert info["n_burned"] == 0
            if name in ("contains the grid", "exactly the extent"):
                assert info["n_burned"] == 67 * 133
            if name == "zero area" and not touches:
                assert info["n_burned"] == 0
    # no feature at all
    run(hip, Features("polygon", np.zeros((0, 2)), [0], [0], np.zeros(0)), g)


def test_overlapping_features_rules_batches_streams_and_the_host_entry(hip):
    import torch
    from machisplin_amd.rasterize import rasterize, c_features
    g = grid(67, 133)
    ft = scene(g, 11)
    wants = {}
    for rule in rr.RULES:
        for touches in (False, True):
            wants[rule, touches] = rr.rasterize(ft, g, rule, touches)
            run(hip, ft, g, rule, touches, want=wants[rule, touches])
        w32 = rr.rasterize(ft, g, rule, False, np.float32)
        run(hip, ft, g, rule, False, dtype="f32", want=w32)
    assert len({wants[r, False][0]["index"].tobytes() for r in rr.RULES}) == 4            # the rules do differ on this scene
    # touches = the centre rule OR the rings as lines
    centre, lines, both = (rr.rasterize(f, g, touches=t)[0]["count"] for f, t in ((ft, False), (ft.rings_as_lines(), False), (ft, True)))
    dev = {k: rasterize(f, g, ("index", "count"), touches=t)[0] for k, (f, t) in {"c": (ft, False), "l": (ft.rings_as_lines(), False), "b": (ft, True)}.items()}
    assert torch.equal(dev["b"]["index"] >= 0, (dev["c"]["index"] >= 0) | (dev["l"]["index"] >= 0)) and ((both > 0) == ((centre > 0) | (lines > 0))).all()
    assert (both >= np.maximum(centre, lines)).all() and (both > centre).any()
    # subsets of the products, in the caller's order; a repeated call gives the same bytes
    run(hip, ft, g, "max", True, products=("value", "index"), want=wants["max", True])
    run(hip, ft, g, "min", False, products=("count",), want=wants["min", False])
    a, _ = rasterize(ft, g, ALL, "max", True)
    b, _ = rasterize(ft, g, ALL, "max", True)
    assert all(a[p].cpu().numpy().tobytes() == b[p].cpu().numpy().tobytes() for p in ALL)
    # the scratch budget: one batch, a few, one per feature -- identical planes.  Every feature here meets the grid, so each has a
    # bit plane (a feature wholly outside has none and shares its neighbour's batch)
    inside = Features.from_parts("polygon", [rr.feature_parts(ft, i) for i in range(3)] +
                                 [[on_grid(g, [u, u + 0.3, u + 0.3, u, u], [0.2, 0.2, 0.7, 0.7, 0.2])] for u in (0.1, 0.25, 0.4, 0.55)], np.arange(7.0))
    want = rr.rasterize(inside, g, "first", True)
    _, one = run(hip, inside, g, "first", True, want=want)
    assert one["n_batches"] == 1
    seen = set()
    for budget in (1 << 20, 2400, 1600, 1):
        _, info = run(hip, inside, g, "first", True, want=want, scratch_budget=budget)
        seen.add(info["n_batches"])
        assert info["scratch_bytes"] <= one["scratch_bytes"]
    assert 1 in seen and len(inside) in seen and any(1 < k < len(inside) for k in seen), seen
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(hip, ft, g, "min", True, want=wants["min", True], stream=side.cuda_stream)
    side.synchronize()
    # the host entry
    for rule, touches, vdt in (("max", True, np.float64), ("last", False, np.float32)):
        want = rr.rasterize(ft, g, rule, touches, vdt)
        index, count, value = np.empty((67, 133), np.int32), np.empty((67, 133), np.int32), np.empty((67, 133), vdt)
        out = _lib.RasterizeOut(index.ctypes.data, count.ctypes.data, value.ctypes.data, 0, 0, 0, _lib.F64 if vdt == np.float64 else _lib.F32)
        info = _lib.RasterizeInfo()
        cg, cf = g.c_struct(), c_features(ft)
        _lib.check(_lib.lib().mhs_rasterize(C.byref(cg), C.byref(cf), rr.RULES.index(rule), int(touches), C.byref(out), 0, C.byref(info)))
        assert bits_equal(index, want[0]["index"]) and bits_equal(count, want[0]["count"]) and bits_equal(value, want[0]["value"])
        assert {k: getattr(info, k) for k in rr.INFO} == want[1]


def segments_for(g, seed):
    """polylines and single segments: random, horizontal, vertical, on cell edges, leaving the grid on each side"""
    rng = np.random.default_rng(seed)
    feats = [[on_grid(g, rng.uniform(0.0, 1.0, 2), rng.uniform(0.0, 1.0, 2))] for _ in range(10)]
    feats.append([on_grid(g, [0.1, 0.9], [0.4, 0.4])])                          # horizontal
    feats.append([on_grid(g, [0.3, 0.3], [0.1, 0.95])])                         # vertical
    feats.append([np.array([[g.xmin + 3 * g.xres, g.ymax - 2 * g.yres], [g.xmin + 3 * g.xres, g.ymax - 9 * g.yres],
                            [g.xmin + 20 * g.xres, g.ymax - 9 * g.yres]])])     # along cell edges
    for u, v in ((-0.3, 0.2), (1.3, 0.6), (0.4, -0.3), (0.7, 1.3)):             # leaving on each side
        feats.append([on_grid(g, [0.5, u], [0.5, v])])
    feats.append([on_grid(g, [-0.2, 1.2], [0.8, 0.75])])                        # right through
    feats.append([on_grid(g, [1.1, 1.4], [0.2, 0.9])])                          # wholly outside
    feats.append([on_grid(g, rng.uniform(0, 1, 40), rng.uniform(0, 1, 40)), on_grid(g, rng.uniform(0, 1, 5), rng.uniform(0, 1, 5))])     # two polylines
    feats.append([on_grid(g, [0.25, 0.25], [0.25, 0.25])])                      # a segment of no length
    return Features.from_parts("line", feats, rng.integers(0, 4, len(feats)).astype(float))


def test_lines_and_points(hip):
    g = grid(67, 133)
    ft = segments_for(g, 21)
    for rule in rr.RULES:
        run(hip, ft, g, rule)
    run(hip, ft, g, "last", scratch_budget=1)
    # points: the east and south edges, the corners, outside; many points to a cell, so that the count atomics collide
    xmax, ymin = g.xmax, g.ymin
    edge = np.array([[g.xmin, g.ymax], [xmax, ymin], [xmax, g.ymax], [g.xmin, ymin], [np.nextafter(xmax, np.inf), 500.0], [g.xmin - 1e-9, 880.0],
                     [150.0, np.nextafter(g.ymax, np.inf)], [150.0, ymin - 1.0], [100.0 + 1.5 * 7, 900.0 - 2.0 * 5], [1e300, -1e300]])
    ft = Features("point", edge, np.arange(11), np.arange(11), np.arange(10.0))
    _, info = run(hip, ft, g, "first")
    assert info["n_outside"] == 5
    g = grid(33, 65)
    rng = np.random.default_rng(4)
    pts = on_grid(g, rng.uniform(-0.05, 1.05, 10000), rng.uniform(-0.05, 1.05, 10000))
    multi = Features("point", pts, np.arange(0, 10001, 4), np.arange(2501), rng.integers(0, 50, 2500).astype(float))      # MultiPoints of four
    for rule in rr.RULES:
        planes, info = run(hip, multi, g, rule)
    assert int(planes["count"].sum()) == 10000 - info["n_outside"] and int(planes["count"].max()) > 3


def _dem(hip):
    """a 60 x 80 tilted, undulating DEM with a sea of NA cells in the south-east, 30 m cells"""
    import torch
    g = Geometry(1000.0, 5000.0, 30.0, 30.0, 60, 80)
    r, c = np.meshgrid(np.arange(60.0), np.arange(80.0), indexing="ij")
    z = 200.0 - 1.5 * r - 1.0 * c + 15.0 * np.sin(c / 6.0) * np.cos(r / 9.0) + np.random.default_rng(31).standard_normal((60, 80))
    z[r + c > 115] = np.nan
    z = z.astype(np.float32)
    return g, z, hip.RasterStack(g, torch.from_numpy(z[None]).cuda(), float("nan"))


def test_composition_with_zonal_proximity_and_covariates(hip):
    import torch
    from machisplin_amd import terrain
    from machisplin_amd.rasterize import rasterize
    g, z, st = _dem(hip)
    units = Features.from_parts("polygon", [[r] for r in rr.lattice(g, 4, 5, 2, zigzag=3)][:-3])          # the last three units are missing
    want_planes, _ = rr.rasterize(units, g)
    # index -> zonal
    zones, _ = rasterize(units, g, ("index",))
    table, planes, _ = hip.zonal.zonal(st, zones["index"], 0, stats=("mean", "count", "cells"), planes=("mean", "minus_mean", "dev"), n_zones=len(units))
    wt, wp, _ = zr.zonal(z, want_planes["index"], n_zones=len(units))
    for k in ("mean", "count", "cells"):
        assert bits_equal(table[k].cpu().numpy(), wt[k]), k
    for k in ("mean", "minus_mean", "dev"):
        assert bits_equal(planes[k].cpu().numpy(), wp[k]), k
    # value -> proximity: the distance to a river
    river = Features.from_parts("line", [[on_grid(g, [0.05, 0.3, 0.5, 0.95], [0.1, 0.4, 0.35, 0.9])]], [1.0])
    burned, _ = rasterize(river, g, ("value",))
    dist = hip.proximity.proximity(hip.RasterStack(g, burned["value"][None], float("nan")), 0, "valid", None, "dist")[0].cpu().numpy()
    on = rr.rasterize(river, g)[0]["index"] >= 0
    rows, cols = np.nonzero(on)
    d2 = ((np.arange(60)[:, None, None] - rows) ** 2 + (np.arange(80)[None, :, None] - cols) ** 2).min(axis=2)
    assert bits_equal(dist, np.sqrt(d2.astype(np.float64)) * 30.0) and (dist[on] == 0).all()
    # the four specs of covariates
    old = ("slope_deg", "twi", "dist_na")
    cov = terrain.covariates(st, old + (("dist_features", river), ("zone_mean", units), ("zone_minus_mean", units), ("zone_dev", units)))
    assert cov.names == ["dem", "slope_deg", "twi", "dist_na", "dist_features", "zone_mean", "zone_minus_mean", "zone_dev"]
    assert cov.planes.dtype == torch.float32
    plain = terrain.covariates(st, old)                                        # an old spec list gives unchanged bytes beside the new specs
    assert plain.planes.cpu().numpy().tobytes() == cov.planes[:4].cpu().numpy().tobytes()
    got = cov.planes.cpu().numpy()
    assert bits_equal(got[4], (np.sqrt(d2.astype(np.float64)) * 30.0).astype(np.float32))
    _, wp32, _ = zr.zonal(z, want_planes["index"], n_zones=len(units), f32=True)
    for k, name in ((5, "mean"), (6, "minus_mean"), (7, "dev")):
        assert bits_equal(got[k], wp32[name]), name
    assert np.isnan(got[5][want_planes["index"] < 0]).all() and (want_planes["index"] < 0).sum() > 100
    one = terrain.covariates(st, (("zone_dev", units),))
    assert one.names == ["dem", "zone_dev"] and bits_equal(one.planes[1].cpu().numpy(), got[7])
    for bad in (("zone_mean",), ("dist_features", 3), ("zone_dev", units, 1)):
        with pytest.raises(ValueError, match=bad[0]):
            terrain.covariates(st, (bad,))


def test_a_partition_of_3600_polygons_on_1500_x_1700(hip):
    g = Geometry(0.0, 1500.0, 1.0, 1.0, 1500, 1700)
    rings = rr.lattice(g, 60, 60, 5)
    ft = Features.from_parts("polygon", [[r] for r in rings], np.arange(3600.0) % 7)
    want = rr.rasterize(ft, g, "last", False)
    assert (want[0]["count"] == 1).all()                                        # shared edges: no gap, no overlap
    run(hip, ft, g, "last", False, want=want)
    run(hip, ft, g, "last", False, products=("index",), want=want, scratch_budget=40000)
