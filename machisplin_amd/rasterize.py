"""Points, lines and polygons burned onto the grid on the device: what ``terra::rasterize`` is used for.

The administrative units or catchments one wants :func:`zonal.zonal` statistics for, the digitised coastline, rivers and lakes
one wants the :func:`proximity.proximity` distance to, the stations' density per cell.  include/machisplin_hip.h, section
"rasterize", states the rule: a polygon covers the cells whose CENTRE lies inside it (even-odd over all rings of the feature), a
line every cell it passes through (4-connected), a point its cell; two polygons that share an edge leave no gap and no overlap.
Every product is an integer or a gather, so every plane equals a numpy restatement exactly and a repeated call gives the same
bytes.  All work on the cells runs in libmachisplin_hip.so (csrc/rasterize.hip); this module only marshals arguments.

Out of scope: partial-coverage fractions, float sums of overlapping features' values, line width and buffers, polygon validity
repair, more than 2^31 - 1 cells, vertices or features.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .vector import KINDS, Features

PRODUCTS = ("index", "count", "value")
RULES = ("last", "first", "max", "min")                                        # MHS_RASTERIZE_LAST, _FIRST, _MAX, _MIN
INT32_MAX = 2 ** 31 - 1
INFO = tuple(k for k, _ in _lib.RasterizeInfo._fields_)


def _check(features, geom, products, rule, out_dtype, scratch_budget):
    """every argument check of :func:`rasterize`, before any device call: (products, scratch_budget)"""
    import torch
    if not isinstance(features, Features):
        raise ValueError("features must be a vector.Features")
    products = (products,) if isinstance(products, str) else tuple(products)
    for p in products:
        if p not in PRODUCTS:
            raise ValueError(f"unknown product {p!r}: one of {', '.join(PRODUCTS)}")
    if len(set(products)) != len(products):
        raise ValueError("products must name each product once")
    if not products:
        raise ValueError("no product requested: products is empty")
    if rule not in RULES:
        raise ValueError(f"unknown rule {rule!r}: one of {', '.join(RULES)}")
    if geom.nrow < 1 or geom.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if geom.nrow * geom.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {geom.nrow * geom.ncol} passes 2^31 - 1")
    if not (np.isfinite([geom.xmin, geom.ymax, geom.xres, geom.yres]).all() and geom.xres > 0 and geom.yres > 0):
        raise ValueError("bad grid geometry: xmin, ymax must be finite, xres, yres positive and finite")
    features.check()
    if features.values is None and "value" in products:
        raise ValueError("values is missing: the value product needs it")
    if features.values is None and rule in ("max", "min"):
        raise ValueError(f"values is missing: the rule {rule!r} needs it")
    if features.values is not None and rule in ("max", "min") and not np.isfinite(features.values).all():
        raise ValueError(f"values must be finite with the rule {rule!r}")
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    if scratch_budget is not None:
        scratch_budget = int(scratch_budget)
        if scratch_budget < 1:
            raise ValueError("scratch_budget must be a positive number of bytes (None: 256 MiB)")
    return products, scratch_budget


def rasterize(features, geom, products=("index",), rule="last", touches=False, out_dtype=None, scratch_budget=None, stream=None, device=None):
    """Burn ``features`` (a :class:`vector.Features` in the grid's coordinate system) onto the grid ``geom``
    (include/machisplin_hip.h, section "rasterize").

    ``products`` names some of :data:`PRODUCTS`: ``index`` (int32: the winning feature, -1 for none -- a ready zone plane for
    :func:`zonal.zonal` with ``n_zones=len(features)``), ``count`` (int32: the number of features that cover the cell; for points
    the number of points in it) and ``value`` (``out_dtype``, float64 unless given: ``values[index]``, NaN for none -- in a
    ``RasterStack`` what ``proximity(where="valid")`` takes).  ``rule`` says which feature wins where several cover a cell:
    ``last`` or ``first`` in the order of the features, ``max`` or ``min`` of ``values`` (ties: the later feature for ``max``,
    the earlier for ``min``).  ``touches=True`` (polygons) adds every cell that a ring passes through to the centre rule.
    ``scratch_budget``: the bytes of per-feature bit planes that one batch of features may take (None: 256 MiB); the planes are
    the same whatever it is.

    Returns ``(planes, info)``: a dict of device tensors by name and a dict of the fields of mhs_rasterize_info (n_features,
    n_parts, n_vertices, n_edges, n_items, n_batches, n_burned, n_outside, scratch_bytes)."""
    import torch
    products, scratch_budget = _check(features, geom, products, rule, out_dtype, scratch_budget)
    out_dtype = out_dtype or torch.float64
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    planes = {p: torch.empty((geom.nrow, geom.ncol), dtype=out_dtype if p == "value" else torch.int32, device=dev) for p in products}
    ptr = lambda p: planes[p].data_ptr() if p in planes else None            # noqa: E731
    out = _lib.RasterizeOut(ptr("index"), ptr("count"), ptr("value"), geom.ncol, geom.ncol, geom.ncol, _lib.F64 if out_dtype == torch.float64 else _lib.F32)
    ft = c_features(features)
    cg = geom.c_struct()
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    info = _lib.RasterizeInfo()
    _lib.check(_lib.lib().mhs_rasterize_dev(C.byref(cg), C.byref(ft), RULES.index(rule), int(bool(touches)), C.byref(out), scratch_budget or 0, st,
                                            C.byref(info)))
    return planes, {k: getattr(info, k) for k in INFO}


def c_features(features):
    """struct mhs_features; it points into the arrays of ``features``, which must outlive the call"""
    return _lib.Features(KINDS.index(features.kind), features.n_vertices, features.n_parts, features.n_features, features.coords.ctypes.data,
                         features.part_offsets.ctypes.data, features.feature_offsets.ctypes.data,
                         None if features.values is None else features.values.ctypes.data)
