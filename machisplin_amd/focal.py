"""Window statistics of one layer at any radius: ``terra::focal`` for sums, moments, min and max, multi-scale covariates from a DEM.

``terrain.relief`` holds its window in LDS and stops at 45 cells; the covariates that act over kilometres -- TPI and DEV at
landscape scale, the standard deviation of elevation, the smoothed "effective terrain" -- need radii of hundreds of cells.
:func:`focal` makes them from blocked prefix sums: O(1) per cell in the radius for a square window, O(R) for a circular one.
include/machisplin_hip.h, section "focal", states the rules; all arithmetic on the cells runs in libmachisplin_hip.so
(csrc/focal.hip).  This module only marshals arguments -- and picks the default ``offset``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .raster import RasterStack
from .terrain import _mask, _planes, _stream, _window

STATS = ("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev")
SHAPES = ("square", "circle")
MINMAX = ("min", "max", "range", "above_min", "below_max")
MAX_RADII = 8


def default_offset(stack: RasterStack, layer=0) -> float:
    """what :func:`focal` centres the values by when ``offset`` is None: the mean of the layer's valid cells rounded to an
    integer (0.0 for a layer without one).  A ``window`` call and the whole-grid call it is compared with must use the
    same offset: pass it on."""
    import torch
    p = stack.planes[layer]
    z = p.to(torch.float64)
    ok = ~torch.isnan(z)
    if stack.nodata == stack.nodata:
        ok &= z != stack.nodata
    n = int(ok.sum())
    return float(torch.round(torch.where(ok, z, torch.zeros_like(z)).sum() / n)) if n else 0.0


def focal(stack: RasterStack, radius, stats="mean", layer=0, shape="square", fill_na=False, window=None, out_dtype=None, out=None,
          stream=None, offset=None):
    """Statistics of layer ``layer`` in the window of ``radius`` cells (1 .. max(nrow, ncol)) around every cell, NA cells and
    cells outside the raster skipped.  ``shape``: ``"square"`` (2 R + 1 cells a side) or ``"circle"`` (``terrain.relief``'s
    window).  ``stats`` names some of :data:`STATS`; ``sd`` is the sample form, ``minus_mean`` = e - mean (TPI at scale),
    ``dev`` = (e - mean) / sd, ``above_min`` = e - min, ``below_max`` = max - e.  A circle gives the sum family only (count, sum,
    mean, sd, minus_mean, dev): ``terrain.relief`` has min and max in a circle up to 45 cells.

    ``radius`` may be a sequence of up to 8 radii: the tables that do not depend on the radius are made once, and the result
    has a leading radius axis.  A device tensor (n_stats, rows, cols) in the order of ``stats`` -- (rows, cols) when
    ``stats`` is one name -- with that leading axis for several radii; NaN where the centre is NA, unless ``fill_na`` makes
    the statistics that do not use the centre there too.  ``window`` = (r0, r1, c0, c1) gives those cells of the whole-grid result bit for bit,
    given the same ``offset`` (the constant the values are centred by before they are squared and summed; None:
    :func:`default_offset` of the layer).  ``out``: a pre-allocated (n_radii * n_stats, rows, cols) tensor for the planes in
    the LIBRARY's order (radius after radius, ascending position in :data:`STATS`)."""
    import torch
    one, names, mask, order = _mask(stats, STATS, "statistic")
    if shape not in SHAPES:
        raise ValueError(f"unknown shape {shape!r}: one of {', '.join(SHAPES)}")
    one_radius = not hasattr(radius, "__len__")
    radii = [int(radius)] if one_radius else [int(r) for r in radius]
    if not 1 <= len(radii) <= MAX_RADII:
        raise ValueError(f"give 1 .. {MAX_RADII} radii, got {len(radii)}")
    bad = [n for n in names if n in MINMAX]
    if bad and shape == "circle":
        raise ValueError(f"a circle window gives the sum family only, not {bad[0]!r}: terrain.relief has min / max in a circle for "
                         f"radius <= 45, shape='square' is meant for them beyond")
    r0, r1, c0, c1 = _window(stack, window)
    if offset is None:
        offset = default_offset(stack, layer)
    n = len(names)
    out, code = _planes(stack, (r1 - r0, c1 - c0), n * len(radii), out_dtype or torch.float64, out)
    g, s = stack.geom.c_struct(), stack.c_struct()
    rad = (C.c_int * len(radii))(*radii)
    _lib.check(_lib.lib().mhs_focal_dev(C.byref(g), C.byref(s), int(layer), rad, len(radii), SHAPES.index(shape), mask, int(bool(fill_na)),
                                        float(offset), r0, r1, c0, c1, out.data_ptr(), code, out.stride(1), out.stride(0), _stream(stack, stream)))
    res = out.unflatten(0, (len(radii), n))
    if order != list(range(n)):
        res = res[:, order]
    if one:
        res = res[:, 0]
    return res[0] if one_radius else res
