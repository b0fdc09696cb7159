"""Vector features as flat arrays: what :func:`rasterize.rasterize` burns onto a grid.

A :class:`Features` holds points, lines or polygons of ONE kind in the layout of ``struct mhs_features``
(include/machisplin_hip.h, section "rasterize"): ``coords`` is ``(V, 2)`` float64 in the grid's coordinate system;
``part_offsets`` (``P + 1`` vertex numbers) cuts it into parts -- a ring of a polygon, a polyline of a line, a run of points --
and ``feature_offsets`` (``F + 1`` part numbers) groups the parts into features, so a polygon with holes or a multi-part feature
is simply a feature of several rings.  :func:`read_geojson` reads the six geometry types of a GeoJSON FeatureCollection with the
standard library's ``json``.

Out of scope: Shapefile, GeoPackage and WKT readers; GeometryCollection; reprojection along curved edges (``transform`` moves
the vertices only); polygon validity repair.
"""
from __future__ import annotations

import json
import math

import numpy as np

KINDS = ("point", "line", "polygon")                                           # MHS_RASTERIZE_POINT, _LINE, _POLYGON


class Features:
    """Points, lines or polygons of one kind (see the module's text).  ``values``: one float64 per feature, or None."""

    def __init__(self, kind, coords, part_offsets, feature_offsets, values=None):
        if kind not in KINDS:
            raise ValueError(f"unknown kind {kind!r}: one of {', '.join(KINDS)}")
        self.kind = kind
        self.coords = np.ascontiguousarray(np.asarray(coords, dtype=np.float64).reshape(-1, 2))
        self.part_offsets = np.ascontiguousarray(part_offsets, dtype=np.int64).reshape(-1)
        self.feature_offsets = np.ascontiguousarray(feature_offsets, dtype=np.int64).reshape(-1)
        self.values = None if values is None else np.ascontiguousarray(values, dtype=np.float64).reshape(-1)

    @property
    def n_vertices(self):
        return self.coords.shape[0]

    @property
    def n_parts(self):
        return max(self.part_offsets.size - 1, 0)

    @property
    def n_features(self):
        return max(self.feature_offsets.size - 1, 0)

    def __len__(self):
        return self.n_features

    @classmethod
    def from_parts(cls, kind, features, values=None):
        """from nested lists: ``features`` is a list of features, each a list of parts, each an ``(n, 2)`` array of vertices"""
        parts = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for f in features for p in f]
        coords = np.concatenate(parts) if parts else np.zeros((0, 2))
        part_offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        feature_offsets = np.concatenate([[0], np.cumsum([len(f) for f in features])]).astype(np.int64)
        return cls(kind, coords, part_offsets, feature_offsets, values)

    def check(self):
        """every refusal of the "rasterize" section that concerns the geometry (ValueError naming the argument)"""
        V, P, F = self.n_vertices, self.n_parts, self.n_features
        if max(V, P, F) > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 vertices, parts or features are out of scope")
        if not np.isfinite(self.coords).all():
            raise ValueError(f"coords holds a non-finite coordinate (vertex {int(np.argwhere(~np.isfinite(self.coords))[0, 0])})")
        for name, off, end, what in (("feature_offsets", self.feature_offsets, P, "n_parts"), ("part_offsets", self.part_offsets, V, "n_vertices")):
            if off.size < 1 or off[0] != 0 or off[-1] != end:
                raise ValueError(f"{name} must start at 0 and end at {what} = {end}")
            if (np.diff(off) < 0).any():
                raise ValueError(f"{name} must not decrease")
        n = np.diff(self.part_offsets)
        if self.kind == "line" and (n < 2).any():
            raise ValueError(f"line part {int(np.argmax(n < 2))} has fewer than 2 vertices")
        if self.kind == "polygon":
            if (n < 4).any():
                raise ValueError(f"ring {int(np.argmax(n < 4))} has fewer than 4 vertices")
            open_ = (self.coords[self.part_offsets[:-1]] != self.coords[self.part_offsets[1:] - 1]).any(axis=1)
            if open_.any():
                raise ValueError(f"ring {int(np.argmax(open_))} is not closed (its last vertex is not its first)")
        if self.values is not None and self.values.size != F:
            raise ValueError(f"values must hold one number per feature ({F}), not {self.values.size}")

    def transform(self, src_crs, dst_crs):
        """the same features with every vertex moved from ``src_crs`` to ``dst_crs`` (:func:`project.transform_points`); the edges
        stay straight between the moved vertices"""
        from . import project
        return Features(self.kind, project.transform_points(self.coords, src_crs, dst_crs), self.part_offsets, self.feature_offsets, self.values)

    def rings_as_lines(self):
        """the rings of polygons as polylines, feature by feature: what ``touches=True`` adds to the centre rule"""
        return Features("line", self.coords, self.part_offsets, self.feature_offsets, self.values)


_GEOJSON = {"Point": ("point", 0), "MultiPoint": ("point", 1), "LineString": ("line", 1), "MultiLineString": ("line", 2), "Polygon": ("polygon", 2),
            "MultiPolygon": ("polygon", 3)}


def read_geojson(path, field=None):
    """The Point / MultiPoint / LineString / MultiLineString / Polygon / MultiPolygon features of a GeoJSON file (a
    FeatureCollection, a Feature or a bare geometry) as ``{kind: Features}``, one entry per kind that occurs, the features of
    a kind in file order.  ``field`` names the numeric property that becomes ``values`` (a feature without it, or with null,
    gets NaN).  A third coordinate is dropped.  Any other geometry type raises ValueError."""
    with open(path, "r", encoding="utf-8") as fh:
        doc = json.load(fh)
    if doc.get("type") == "FeatureCollection":
        items = doc.get("features", [])
    elif doc.get("type") == "Feature":
        items = [doc]
    else:
        items = [{"type": "Feature", "geometry": doc, "properties": {}}]
    parts = {k: [] for k in KINDS}
    values = {k: [] for k in KINDS}
    for n, item in enumerate(items):
        geom = item.get("geometry") or {}
        gtype = geom.get("type")
        if gtype not in _GEOJSON:
            raise ValueError(f"feature {n}: geometry type {gtype!r} is out of scope (one of {', '.join(_GEOJSON)})")
        kind, depth = _GEOJSON[gtype]
        c = geom.get("coordinates", [])
        if depth == 0:
            rings = [[c]]
        elif depth == 1:
            rings = [c]
        elif depth == 2:
            rings = list(c)
        else:
            rings = [ring for poly in c for ring in poly]
        parts[kind].append([np.asarray(r, dtype=np.float64).reshape(len(r), -1)[:, :2] for r in rings])
        v = (item.get("properties") or {}).get(field) if field is not None else None
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
            raise ValueError(f"feature {n}: property {field!r} is not a number")
        values[kind].append(math.nan if v is None else float(v))
    return {k: Features.from_parts(k, parts[k], values[k] if field is not None else None) for k in KINDS if parts[k]}
