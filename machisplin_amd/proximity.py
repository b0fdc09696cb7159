"""Distance-to-feature covariates: exact Euclidean proximity on the device.

Distance to the coast, to open water, to the channel network -- the covariates an ANUSPLIN-style interpolation uses next to
elevation, and for which the reference's users go to ``terra::distance`` -- with the index of the nearest feature cell, from
which the direction to it and the value of another layer there follow.  include/machisplin_hip.h, section "proximity", states
the rule: squared distances and the tie rule are exact integers, so every plane equals a numpy restatement bit for bit.  All
arithmetic on the cells runs in libmachisplin_hip.so (csrc/proximity.hip); this module only marshals arguments.

Out of scope: non-square cells, geodesic distance on lon/lat grids (there the result is in degrees times ``unit``), cost or
path distance, a search radius cap.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .raster import Geometry

WHERE = ("na", "valid", "lt", "le", "gt", "ge", "eq", "ne")                    # the MHS_PROX_* of the header, in its order
PRODUCTS = ("d2", "index", "dist", "dir_x", "dir_y", "value")                  # the planes of mhs_proximity_out, in its order
INT32_MAX = 2 ** 31 - 1


class ProximityResult(dict):
    """what :func:`proximity` returns for several products: the planes by name, and ``.info``"""
    info = None


class _Plane:
    """a 2-D tensor of feature flags in the place of a RasterStack: one float32 layer, 1 at the features and 0 elsewhere"""

    def __init__(self, mask):
        import torch
        self.geom = Geometry(0.0, float(mask.shape[0]), 1.0, 1.0, int(mask.shape[0]), int(mask.shape[1]))
        self.nodata = float("nan")
        self.n_layers = 1
        self._mask = mask
        self._torch = torch

    @property
    def planes(self):
        dev = self._torch.device("cuda", _lib.init())
        return (self._mask.to(dev) != 0).to(self._torch.float32)[None].contiguous()


def _check(stack, layer, where, threshold, products, value_layer, unit, out_dtype):
    """every argument check of :func:`proximity`, before any device call: (stack, where code, threshold, names, unit)"""
    import torch
    if isinstance(stack, torch.Tensor):
        if stack.dim() != 2 or stack.dtype.is_floating_point or stack.dtype.is_complex:
            raise ValueError("stack must be a RasterStack or a 2-D bool or integer tensor of feature flags")
        if where != "na" or threshold is not None or layer != 0:
            raise ValueError("a tensor of feature flags takes no layer, where or threshold: every nonzero cell is a feature")
        stack, where, threshold = _Plane(stack), "ne", 0.0
    if where not in WHERE:
        raise ValueError(f"unknown where {where!r}: one of {', '.join(WHERE)}")
    code = WHERE.index(where)
    if code >= 2:
        if threshold is None:
            raise ValueError(f"where={where!r} needs a threshold")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
    else:
        threshold = 0.0
    one = isinstance(products, str)
    names = (products,) if one else tuple(products)
    for n in names:
        if n not in PRODUCTS:
            raise ValueError(f"unknown product {n!r}: one of {', '.join(PRODUCTS)}")
    if not names or len(set(names)) != len(names):
        raise ValueError("products must name at least one product, each once")
    g = stack.geom
    if not 0 <= int(layer) < stack.n_layers:
        raise ValueError(f"layer {layer} is not one of the stack's {stack.n_layers} layers")
    if "value" in names:
        if value_layer is None:
            raise ValueError("the value product needs value_layer, the layer whose value at the nearest feature is wanted")
        if not 0 <= int(value_layer) < stack.n_layers:
            raise ValueError(f"value_layer {value_layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if (g.nrow - 1) ** 2 + (g.ncol - 1) ** 2 > INT32_MAX:
        raise ValueError(f"grid too large: (nrow - 1)^2 + (ncol - 1)^2 = {(g.nrow - 1) ** 2 + (g.ncol - 1) ** 2} passes 2^31 - 1 (d2 is an int32)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1 (index is an int32)")
    if unit is None:
        if abs(g.xres - g.yres) > 1e-9 * max(abs(g.xres), abs(g.yres)):
            raise ValueError(f"unit: the cells are not square (xres {g.xres}, yres {g.yres}); bring the raster onto a square grid "
                             "with resample.resample, or give unit explicitly")
        unit = g.xres
    unit = float(unit)
    if not (unit > 0.0 and unit != float("inf")):
        raise ValueError("unit must be finite and positive")
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    return stack, code, threshold, one, names, unit


def proximity(stack, layer=0, where="na", threshold=None, products=("dist",), value_layer=None, unit=None, out_dtype=None, stream=None):
    """The nearest feature of every cell of layer ``layer`` (include/machisplin_hip.h, section "proximity").  A cell is a
    feature when it satisfies ``where``, one of :data:`WHERE`: ``na`` (NaN or the stack's nodata: the sea of a land-only
    DEM), ``valid``, or ``lt le gt ge eq ne`` against ``threshold``.  ``products`` names some of :data:`PRODUCTS`: ``d2``
    (int32, squared distance in cells, exact), ``index`` (int32, the nearest feature's cell number row * ncol + col; ties go
    to the smaller row, then the smaller column), ``dist`` = sqrt(d2) * ``unit``, ``dir_x`` / ``dir_y`` (the unit vector
    towards the feature, y positive to the north, 0 at a feature) and ``value`` (layer ``value_layer`` at the nearest
    feature).  Without any feature d2 and index are -1 and the float products NaN.

    ``unit`` = None takes the geometry's cell width and raises ValueError when width and height differ by more than 1e-9
    relative (see ``resample``); an explicit ``unit`` skips that check.  Always the whole plane: there is no window.
    A 2-D bool or integer tensor may stand in place of ``stack``: every nonzero cell is a feature (``unit`` defaults to 1).

    Returns ``(planes, info)``: a dict of device tensors by name (``.info`` too) -- or the single tensor when ``products`` is
    one name -- and a dict of the fields of mhs_proximity_info (n_features, max_d2, scratch_bytes)."""
    import torch
    stack, code, threshold, one, names, unit = _check(stack, layer, where, threshold, products, value_layer, unit, out_dtype)
    out_dtype = out_dtype or torch.float64
    g = stack.geom
    src = stack.planes
    planes = {n: torch.empty((g.nrow, g.ncol), dtype=torch.int32 if n in ("d2", "index") else out_dtype, device=src.device) for n in names}
    out = _lib.ProximityOut(*[planes[n].data_ptr() if n in planes else None for n in PRODUCTS])
    info = _lib.ProximityInfo()
    cg = g.c_struct()
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    cs = _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)
    st = stream if stream is not None else torch.cuda.current_stream(src.device).cuda_stream
    _lib.check(_lib.lib().mhs_proximity_dev(C.byref(cg), C.byref(cs), int(layer), code, threshold, int(value_layer) if value_layer is not None else -1,
                                            unit, C.byref(out), _lib.F64 if out_dtype == torch.float64 else _lib.F32, g.ncol, st, C.byref(info)))
    info = {k: getattr(info, k) for k, _ in _lib.ProximityInfo._fields_}
    if one:
        return planes[names[0]], info
    res = ProximityResult(planes)
    res.info = info
    return res, info
