"""CPU: the rasterize rule (include/machisplin_hip.h, section "rasterize").  The restatement the GPU tests compare with
(tests/rasterize_ref.py) agrees with matplotlib's point-in-path test on stars with holes and multi-part features, leaves no gap
and no overlap between polygons that share edges, burns for a line exactly the cells whose open interior the segment crosses
(an exact rational Liang-Barsky test with ``fractions``) in one 4-connected piece, and puts points where Geometry's
``row_from_y`` / ``col_from_x`` put them; every entry point refuses bad arguments before it touches a device, naming the argument;
and the rule header the kernels are built from (csrc/rasterize_rule.h) holds against brute-force counts in a plain C++ program
compiled with gcc under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rasterize_ref as rr
from machisplin_amd import _lib
from machisplin_amd import rasterize as rz
from machisplin_amd import vector
from machisplin_amd.raster import Geometry
from machisplin_amd.vector import Features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = Geometry(100.0, 900.0, 1.5, 2.0, 67, 133)                                  # every edge of every cell is exact in float64
NAN = float("nan")


def centres(g):
    grid = rr.Grid(g)
    xx, yy = np.meshgrid(grid.xc, grid.yr)
    return np.column_stack([xx.ravel(), yy.ravel()])


def near_an_edge(g, pts, rings, tol):
    """the cells whose centre lies within tol * res of an edge of a ring (distance in cells)"""
    near = np.zeros(len(pts), dtype=bool)
    scale = np.array([g.xres, g.yres])
    p = pts / scale
    for ring in rings:
        a, b = ring[:-1] / scale, ring[1:] / scale
        for a_, b_ in zip(a, b):
            d = b_ - a_
            L2 = float(d @ d)
            t = np.clip(((p - a_) @ d) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(p))
            near |= np.hypot(*(p - (a_ + t[:, None] * d)).T) < tol
    return near


def test_the_restatement_against_matplotlib_on_stars_with_holes_and_parts():
    from matplotlib.path import Path
    pts = centres(G)
    cx, cy = G.xmin + 0.5 * G.ncol * G.xres, G.ymax - 0.5 * G.nrow * G.yres
    total = left_out = 0
    for seed in range(1, 7):
        rings = [rr.star(cx, cy, 30.0, 60.0, 40, seed), rr.star(cx, cy, 5.0, 25.0, 8, seed + 100),                   # a star and its hole
                 rr.star(cx - 70.0, cy + 30.0, 4.0, 22.0, 12, seed + 200), rr.star(cx + 60.0, cy - 40.0, 3.0, 20.0, 9, seed + 300)]      # two more parts
        ft = Features.from_parts("polygon", [rings])
        planes, info = rr.rasterize(ft, G)
        inside = np.zeros(len(pts), dtype=bool)
        for ring in rings:
            inside ^= Path(ring).contains_points(pts)
        skip = near_an_edge(G, pts, rings, 1e-9)
        got = (planes["index"] >= 0).ravel()
        assert ((got != inside) & ~skip).sum() == 0, seed
        assert got.sum() > 1500 and info["n_burned"] == got.sum() and (planes["count"] == (planes["index"] >= 0)).all()
        total += len(pts)
        left_out += int(skip.sum())
    assert left_out <= 0.001 * total


def test_polygons_that_share_edges_leave_no_gap_and_no_overlap():
    for seed, ny, nx, zigzag in ((1, 5, 7, 0), (2, 6, 4, 5), (3, 1, 2, 23)):
        rings = rr.lattice(G, ny, nx, seed, zigzag=zigzag)
        ft = Features.from_parts("polygon", [[r] for r in rings])
        planes, _ = rr.rasterize(ft, G)
        assert (planes["count"] == 1).all(), (seed, int((planes["count"] == 0).sum()), int((planes["count"] > 1).sum()))
        # the union is the outer rectangle's own fill; each polygon on its own covers what it wins
        xmax, ymin = G.xmax, G.ymin
        outer = Features.from_parts("polygon", [[np.array([[G.xmin, G.ymax], [xmax, G.ymax], [xmax, ymin], [G.xmin, ymin], [G.xmin, G.ymax]])]])
        assert ((rr.rasterize(outer, G)[0]["index"] >= 0) == (planes["index"] >= 0)).all()
        for i in (0, len(rings) - 1):
            alone = rr.rasterize(Features.from_parts("polygon", [[rings[i]]]), G)[0]["index"] >= 0
            assert (alone == (planes["index"] == i)).all()
    # a polygon half outside the grid next to one inside: still no overlap
    big = Geometry(G.xmin - 30.0, G.ymax + 20.0, G.xres, G.yres, G.nrow + 20, G.ncol + 40)
    rings = rr.lattice(big, 4, 4, 9, zigzag=3)
    planes, _ = rr.rasterize(Features.from_parts("polygon", [[r] for r in rings]), G)
    assert (planes["count"] == 1).all()


def crosses_open_cell(p0, p1, x0, x1, y0, y1):
    """exact: does the closed segment p0 p1 meet the open rectangle (x0, x1) x (y0, y1)?  Liang-Barsky in rationals"""
    lo, hi = Fraction(0), Fraction(1)
    strict_lo = strict_hi = False                                                     # is the bound an open one?
    for p, d, a, b in ((p0[0], p1[0] - p0[0], x0, x1), (p0[1], p1[1] - p0[1], y0, y1)):
        if d == 0:
            if not a < p < b:
                return False
            continue
        t0, t1 = (a - p) / d, (b - p) / d
        if t0 > t1:
            t0, t1 = t1, t0
        if t0 >= lo:
            lo, strict_lo = t0, True
        if t1 <= hi:
            hi, strict_hi = t1, True
    return lo < hi or (lo == hi and not strict_lo and not strict_hi)


def exact_cells(g, p0, p1):
    f = lambda v: Fraction(float(v))                                                  # noqa: E731
    p0, p1 = (f(p0[0]), f(p0[1])), (f(p1[0]), f(p1[1]))
    out = np.zeros((g.nrow, g.ncol), dtype=bool)
    xe = [f(g.xmin) + c * f(g.xres) for c in range(g.ncol + 1)]
    ye = [f(g.ymax) - r * f(g.yres) for r in range(g.nrow + 1)]
    xs, ys = sorted((p0[0], p1[0])), sorted((p0[1], p1[1]))
    for r in range(g.nrow):
        if ye[r + 1] > ys[1] or ye[r] < ys[0]:
            continue
        for c in range(g.ncol):
            if xe[c] > xs[1] or xe[c + 1] < xs[0]:
                continue
            out[r, c] = crosses_open_cell(p0, p1, xe[c], xe[c + 1], ye[r + 1], ye[r])
    return out


def components4(mask):
    """the number of 4-connected components of a small mask"""
    todo = set(map(tuple, np.argwhere(mask)))
    n = 0
    while todo:
        n += 1
        stack = [todo.pop()]
        while stack:
            r, c = stack.pop()
            for q in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
                if q in todo:
                    todo.remove(q)
                    stack.append(q)
    return n


def test_the_line_rule_against_the_exact_rational_test():
    rng = np.random.default_rng(1)
    u, v = rng.uniform(0.02, 0.98, (10, 2)), rng.uniform(0.02, 0.98, (10, 2))
    segs = [np.array([[G.xmin + a[0] * 199.5, G.ymax - b[0] * 134.0], [G.xmin + a[1] * 199.5, G.ymax - b[1] * 134.0]]) for a, b in zip(u, v)]
    segs.append(np.array([[111.3, 801.7], [260.9, 801.7]]))                           # horizontal
    segs.append(np.array([[171.2, 890.1], [171.2, 775.3]]))                           # vertical
    segs += [np.array([[200.3, 830.7], [q[0], q[1]]]) for q in ((60.3, 815.2), (340.7, 845.9), (215.1, 930.4), (190.6, 740.2))]      # leaving on each side
    segs.append(np.array([[80.3, 700.9], [331.1, 951.7]]))                            # right through, both ends outside
    burned_all = 0
    for k, s in enumerate(segs):
        planes, info = rr.rasterize(Features.from_parts("line", [[s]]), G)
        burned = planes["index"] >= 0
        want = exact_cells(G, s[0], s[1])
        assert (want & ~burned).sum() == 0 and (burned & ~want).sum() == 0, (k, int((want & ~burned).sum()), int((burned & ~want).sum()))
        assert components4(burned) == 1 and (planes["count"] == burned).all()
        for x, y in s:                                                                # an endpoint inside the grid: its cell is burned
            r, c = int(G.row_from_y(y)), int(G.col_from_x(x))
            if r >= 0 and c >= 0:
                assert burned[r, c], (k, r, c)
        burned_all += int(burned.sum())
    assert burned_all > 900
    # a polyline is one piece, and a feature counts once where its segments share a cell
    line = np.column_stack([G.xmin + rng.uniform(0.05, 0.95, 30) * 199.5, G.ymax - rng.uniform(0.05, 0.95, 30) * 134.0])
    planes, _ = rr.rasterize(Features.from_parts("line", [[line]]), G)
    assert components4(planes["index"] >= 0) == 1 and planes["count"].max() == 1
    union = np.zeros((G.nrow, G.ncol), dtype=bool)
    for a, b in zip(line[:-1], line[1:]):
        union |= exact_cells(G, a, b)
    assert ((planes["index"] >= 0) == union).all()
    # segments along cell edges and of no length: col() and row() put them in the cell to the east and south of the edge
    planes, _ = rr.rasterize(Features.from_parts("line", [[np.array([[103.0, 896.0], [103.0, 890.0]])], [np.array([[109.0, 880.0], [109.0, 880.0]])]]), G)
    assert np.argwhere(planes["index"] >= 0).tolist() == [[2, 2], [3, 2], [4, 2], [5, 2], [10, 6]]


def test_points_against_the_geometry():
    rng = np.random.default_rng(2)
    pts = np.column_stack([rng.uniform(G.xmin - 20.0, G.xmax + 20.0, 4000), rng.uniform(G.ymin - 20.0, G.ymax + 20.0, 4000)])
    pts[:6] = [[G.xmax, 850.0], [150.0, G.ymin], [G.xmax, G.ymin], [G.xmin, G.ymax], [np.nextafter(G.xmax, np.inf), 850.0], [150.0, np.nextafter(G.ymin, -np.inf)]]
    ft = Features("point", pts, np.arange(4001), np.arange(4001))
    planes, info = rr.rasterize(ft, G, "first")
    r, c = G.row_from_y(pts[:, 1]), G.col_from_x(pts[:, 0])
    inside = (r >= 0) & (c >= 0)
    assert inside[:4].all() and not inside[4:6].any() and info["n_outside"] == int((~inside).sum()) and info["n_items"] == 4000
    count = np.zeros((G.nrow, G.ncol), dtype=np.int32)
    first = np.full((G.nrow, G.ncol), -1, dtype=np.int32)
    for i in np.flatnonzero(inside)[::-1]:
        count[r[i], c[i]] += 1
        first[r[i], c[i]] = i
    assert (planes["count"] == count).all() and (planes["index"] == first).all() and count.max() > 1
    assert planes["index"][66, 132] == 2 and planes["index"][0, 0] == 3


def test_key_rules_on_overlapping_features_with_tied_values():
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]])      # noqa: E731
    ft = Features.from_parts("polygon", [[sq(110.0, 880.0, 200.0, 820.0)], [sq(150.0, 860.0, 250.0, 800.0)], [sq(170.0, 870.0, 230.0, 780.0)],
                                         [sq(175.0, 855.0, 195.0, 845.0)]], [2.0, 5.0, 5.0, 2.0])
    common = (int(G.row_from_y(850.0)), int(G.col_from_x(185.0)))                    # inside all four
    won = {rule: rr.rasterize(ft, G, rule) for rule in rr.RULES}
    assert [int(won[rule][0]["index"][common]) for rule in rr.RULES] == [3, 0, 2, 0]      # last, first, max (ties: the later), min (ties: the earlier)
    assert won["max"][0]["value"][common] == 5.0 and won["min"][0]["value"][common] == 2.0
    for rule in rr.RULES:
        planes = won[rule][0]
        assert planes["count"][common] == 4 and (planes["count"] == won["last"][0]["count"]).all()
        assert (np.isnan(planes["value"]) == (planes["index"] < 0)).all() and ((planes["index"] < 0) == (planes["count"] == 0)).all()
        keys = rr.keys_of(4, rule, ft.values)
        assert sorted(keys.tolist()) == [0, 1, 2, 3]                                 # unique
    assert rr.keys_of(4, "max", ft.values).tolist() == [0, 2, 3, 1] and rr.keys_of(4, "min", ft.values).tolist() == [3, 1, 0, 2]
    where12 = (won["last"][0]["count"] == 2) & (won["first"][0]["index"] == 1)      # features 1 and 2 only
    assert where12.any() and (won["max"][0]["index"][where12] == 2).all() and (won["min"][0]["index"][where12] == 1).all()


def test_geojson_every_geometry_type_round_trips(tmp_path):
    ring = [[110.0, 880.0], [200.0, 880.0], [200.0, 820.0], [110.0, 880.0]]
    hole = [[150.0, 870.0], [180.0, 870.0], [180.0, 850.0], [150.0, 870.0]]
    far = [[[210.0, 800.0], [260.0, 800.0], [260.0, 780.0], [210.0, 800.0]]]
    doc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"pop": 3, "name": "a"}, "geometry": {"type": "Point", "coordinates": [120.0, 870.0]}},
        {"type": "Feature", "properties": {"pop": 4.5}, "geometry": {"type": "Polygon", "coordinates": [ring, hole]}},
        {"type": "Feature", "properties": {"pop": None}, "geometry": {"type": "MultiPoint", "coordinates": [[130.0, 860.0, 12.0], [131.0, 861.0, 13.0]]}},
        {"type": "Feature", "properties": {"pop": 7}, "geometry": {"type": "LineString", "coordinates": [[110.0, 800.0], [150.0, 810.0], [170.0, 790.0]]}},
        {"type": "Feature", "properties": {}, "geometry": {"type": "MultiPolygon", "coordinates": [[ring, hole], far]}},
        {"type": "Feature", "properties": {"pop": -1}, "geometry": {"type": "MultiLineString", "coordinates": [[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0], [9.0, 1.0]]]}},
    ]}
    path = tmp_path / "units.geojson"
    path.write_text(json.dumps(doc))
    got = vector.read_geojson(str(path), field="pop")
    assert sorted(got) == ["line", "point", "polygon"]
    pt, ln, pg = got["point"], got["line"], got["polygon"]
    assert pt.coords.tolist() == [[120.0, 870.0], [130.0, 860.0], [131.0, 861.0]] and pt.part_offsets.tolist() == [0, 1, 3] and pt.feature_offsets.tolist() == [0, 1, 2]
    assert pt.values[0] == 3.0 and np.isnan(pt.values[1])
    assert ln.part_offsets.tolist() == [0, 3, 5, 8] and ln.feature_offsets.tolist() == [0, 1, 3] and ln.values.tolist() == [7.0, -1.0]
    assert pg.part_offsets.tolist() == [0, 4, 8, 12, 16, 20] and pg.feature_offsets.tolist() == [0, 2, 5] and pg.values[0] == 4.5 and np.isnan(pg.values[1])
    assert pg.coords[:4].tolist() == ring and pg.coords[16:].tolist() == far[0]
    for ft in got.values():
        ft.check()
    assert vector.read_geojson(str(path))["polygon"].values is None
    # the polygon with its hole equals the first two rings of the multi-polygon; the restatement sees the same cells
    a = rr.rasterize(Features.from_parts("polygon", [rr.feature_parts(pg, 0)]), G)[0]["index"] >= 0
    b = rr.rasterize(pg, G, "first")[0]
    assert a.sum() > 100 and (a == (b["index"] == 0)).all() and (b["count"][a] == 2).all()
    # a bare geometry and a single feature; what is out of scope is named
    path.write_text(json.dumps(doc["features"][3]["geometry"]))
    assert vector.read_geojson(str(path))["line"].n_vertices == 3
    path.write_text(json.dumps(doc["features"][1]))
    assert vector.read_geojson(str(path), "pop")["polygon"].values.tolist() == [4.5]
    path.write_text(json.dumps({"type": "Feature", "properties": {}, "geometry": {"type": "GeometryCollection", "geometries": []}}))
    with pytest.raises(ValueError, match="GeometryCollection"):
        vector.read_geojson(str(path))
    path.write_text(json.dumps({"type": "Feature", "properties": {"pop": "many"}, "geometry": {"type": "Point", "coordinates": [1.0, 2.0]}}))
    with pytest.raises(ValueError, match="not a number"):
        vector.read_geojson(str(path), "pop")


def test_transform_moves_the_vertices():
    from machisplin_amd import project
    src, dst = project.LONLAT, project.utm(18, south=True)
    ft = Features.from_parts("line", [[np.array([[-77.0, -4.0], [-76.5, -4.2]])]], [1.0])
    moved = ft.transform(src, dst)
    assert moved.kind == "line" and moved.part_offsets.tolist() == [0, 2] and moved.values.tolist() == [1.0]
    assert np.array_equal(moved.coords, project.transform_points(ft.coords, src, dst)) and 270000.0 < moved.coords[0, 0] < 285000.0


RING = np.array([[110.0, 880.0], [200.0, 880.0], [200.0, 820.0], [110.0, 880.0]])


def test_refusals_of_the_python_call_come_before_any_device_call(monkeypatch):
    import torch
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called before the refusal")))
    good = Features.from_parts("polygon", [[RING]], [1.0])

    def refused(needle, ft=good, g=G, **kw):
        with pytest.raises(ValueError, match=needle):
            rz.rasterize(ft, g, **kw)

    bad = RING.copy()
    bad[1, 0] = NAN
    refused("non-finite", Features.from_parts("polygon", [[bad]]))
    bad[1, 0] = np.inf
    refused("non-finite", Features.from_parts("polygon", [[bad]]))
    refused("part_offsets must not decrease", Features("polygon", np.vstack([RING, RING]), [0, 5, 4, 8], [0, 3]))
    refused("part_offsets must start at 0 and end at n_vertices", Features("polygon", RING, [0, 3], [0, 1]))
    refused("part_offsets must start at 0", Features("polygon", RING, [1, 4], [0, 1]))
    refused("feature_offsets must start at 0 and end at n_parts", Features("polygon", RING, [0, 4], [0, 2]))
    refused("feature_offsets must not decrease", Features("polygon", np.vstack([RING, RING]), [0, 4, 8], [0, 2, 1, 2]))
    refused("fewer than 4", Features.from_parts("polygon", [[RING[[0, 1, 0]]]]))
    refused("not closed", Features.from_parts("polygon", [[RING[[0, 1, 2, 1]]]]))
    refused("fewer than 2", Features.from_parts("line", [[RING[:1]]]))
    refused(r"nrow \* ncol", g=Geometry(0.0, 0.0, 1.0, 1.0, 46341, 46341))
    refused("grid geometry", g=Geometry(0.0, 0.0, 0.0, 1.0, 10, 10))
    refused("no product", products=())
    refused("unknown product", products=("index", "cover"))
    refused("once", products=("index", "index"))
    refused("values is missing", Features.from_parts("polygon", [[RING]]), products=("value",))
    refused("values is missing", Features.from_parts("polygon", [[RING]]), rule="max")
    refused("values is missing", Features.from_parts("polygon", [[RING]]), rule="min")
    refused("finite", Features.from_parts("polygon", [[RING]], [NAN]), rule="min")
    refused("one number per feature", Features.from_parts("polygon", [[RING]], [1.0, 2.0]))
    refused("unknown rule", rule="sum")
    refused("out_dtype", products=("value",), out_dtype=torch.float16)
    refused("scratch_budget", scratch_budget=0)
    refused("vector.Features", ft=RING)
    with pytest.raises(ValueError, match="unknown kind"):
        Features("surface", RING, [0, 4], [0, 1])


class _Call:
    """One of the two entry points on a 10 x 12 grid.  A refusal comes before the first device call.  The calls that PASS the
    checks end at MHS_ERR_NODEVICE on a machine without a GPU -- where there is one they run, so the planes of the _dev entry are
    then device tensors."""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        self.fn = fn
        if fn.endswith("_dev") and torch.cuda.is_available():
            self.planes = torch.zeros((3, 10, 12), dtype=torch.float64, device="cuda")
            self.ptr = [self.planes[k].data_ptr() for k in range(3)]
        else:
            self.planes = np.zeros((3, 10, 12), dtype=np.float64)
            self.ptr = [self.planes[k].ctypes.data for k in range(3)]
        self.coords = np.array([[1.0, 9.0], [8.0, 9.0], [8.0, 2.0], [1.0, 9.0], [2.0, 3.0], [3.0, 3.0], [3.0, 2.0], [2.0, 3.0]])
        self.parts = np.array([0, 4, 8], dtype=np.int64)
        self.feats = np.array([0, 1, 2], dtype=np.int64)
        self.values = np.array([1.0, 2.0])

    def features(self, kind=2, coords=None, parts=None, feats=None, values="default", n=None):
        self.keep = [np.ascontiguousarray(self.coords if coords is None else coords, dtype=np.float64),
                     np.ascontiguousarray(self.parts if parts is None else parts, dtype=np.int64),
                     np.ascontiguousarray(self.feats if feats is None else feats, dtype=np.int64),
                     None if values is None else np.ascontiguousarray(self.values if isinstance(values, str) else values, dtype=np.float64)]
        c, p, f, v = self.keep
        nv, np_, nf = n if n is not None else (c.shape[0], p.size - 1, f.size - 1)
        return _lib.Features(kind, nv, np_, nf, c.ctypes.data, p.ctypes.data, f.ctypes.data, None if v is None else v.ctypes.data)

    def __call__(self, grid=(0.0, 10.0, 1.0, 1.0, 10, 12), features="default", rule=0, touches=0, out="default", budget=0):
        g = C.byref(_lib.Grid(*grid)) if grid is not None else None
        ft = C.byref(self.features()) if isinstance(features, str) else (C.byref(features) if features is not None else None)
        o = C.byref(_lib.RasterizeOut(self.ptr[0], self.ptr[1], self.ptr[2], 12, 12, 12, _lib.F64)) if isinstance(out, str) else (C.byref(out) if out is not None else None)
        f = getattr(self.lib, self.fn)
        rc = f(g, ft, rule, touches, o, budget, None, None) if self.fn.endswith("_dev") else f(g, ft, rule, touches, o, budget, None)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_rasterize_dev", "mhs_rasterize"))
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", features=None)
    refused("NULL", out=None)
    refused("nrow, ncol", grid=(0.0, 10.0, 1.0, 1.0, 0, 12))
    refused("nrow * ncol", grid=(0.0, 10.0, 1.0, 1.0, 46341, 46341))
    for bad in ((NAN, 10.0, 1.0, 1.0), (0.0, np.inf, 1.0, 1.0), (0.0, 10.0, 0.0, 1.0), (0.0, 10.0, 1.0, -1.0), (0.0, 10.0, NAN, 1.0)):
        refused("grid geometry", grid=bad + (10, 12))
    refused("unknown kind", features=call.features(kind=3))
    refused("unknown rule", rule=4)
    refused("unknown rule", rule=-1)
    refused("no product", out=_lib.RasterizeOut(None, None, None, 12, 12, 12, _lib.F64))
    refused("value_dtype", out=_lib.RasterizeOut(None, None, call.ptr[2], 12, 12, 12, _lib.I16))
    refused("scratch_budget", budget=-1)
    coords = call.coords.copy()
    coords[5, 1] = NAN
    refused("non-finite coordinate (vertex 5)", features=call.features(coords=coords))
    coords[5, 1] = -np.inf
    refused("non-finite", features=call.features(coords=coords))
    refused("part_offsets must not decrease", features=call.features(parts=[0, 5, 4, 8], feats=[0, 1, 3]))
    refused("part_offsets must start at 0 and end at n_vertices", features=call.features(parts=[0, 4, 7]))
    refused("part_offsets must start at 0", features=call.features(parts=[1, 4, 8]))
    refused("feature_offsets must start at 0 and end at n_parts", features=call.features(feats=[0, 1, 3]))
    refused("feature_offsets must start at 0", features=call.features(feats=[1, 1, 2]))
    refused("feature_offsets must not decrease", features=call.features(feats=[0, 2, 1, 2]))
    refused("ring 1 has fewer than 4", features=call.features(coords=call.coords[:7], parts=[0, 4, 7]))
    refused("ring 0 is not closed", features=call.features(coords=call.coords[[0, 1, 2, 1, 4, 5, 6, 4]]))
    refused("line part 1 has fewer than 2", features=call.features(kind=1, parts=[0, 7, 8]))
    refused("values is missing: the value", features=call.features(values=None))
    refused("values is missing: the rules", features=call.features(values=None), rule=2, out=_lib.RasterizeOut(call.ptr[0], None, None, 12, 12, 12, _lib.F64))
    refused("values must be finite", features=call.features(values=[1.0, NAN]), rule=3)
    refused("n_vertices", features=call.features(n=(-1, 2, 2)))
    refused("n_vertices", features=call.features(n=(2 ** 31, 2, 2)))
    if fn.endswith("_dev"):
        refused("ld_index", out=_lib.RasterizeOut(call.ptr[0], None, None, 11, 12, 12, _lib.F64))
        refused("ld_count", out=_lib.RasterizeOut(None, call.ptr[1], None, 12, 11, 12, _lib.F64))
        refused("ld_value", out=_lib.RasterizeOut(None, None, call.ptr[2], 12, 12, 11, _lib.F64))
    for kw in (dict(), dict(rule=2, touches=1), dict(features=call.features(kind=1)), dict(features=call.features(kind=0), rule=3),
               dict(features=call.features(values=None), out=_lib.RasterizeOut(call.ptr[0], call.ptr[1], None, 12, 12, 12, _lib.F64)),
               dict(features=call.features(values=[NAN, 1.0])), dict(budget=1),
               dict(features=call.features(coords=np.zeros((0, 2)), parts=[0], feats=[0], values=[]))):
        rc, msg = call(**kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rasterize_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "rasterize_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK" and int(lines[-2].split()[1]) > 10 ** 6
