"""Flow-path covariates: what lies downstream of a cell along the D8 direction forest.

Height above and distance to the first channel cell that a cell's OWN water meets (HAND; SAGA's vertical and horizontal distance
to channel network), the distance to the outlet, and the catchment a cell drains to -- where ``proximity`` takes the stream cell
nearest as the crow flies, which on a ridge is often one of the wrong catchment.  include/machisplin_hip.h, section "flow
paths", states the rule: pointers and step counts are exact integers and every float product is a few operations rounded once,
so every plane equals a numpy restatement bit for bit.  All arithmetic on the cells runs in libmachisplin_hip.so
(csrc/flowpath.hip: pointer doubling); this module only marshals arguments.

Out of scope: ``dist`` on lon/lat grids (a cell width per row), Strahler order, the longest upstream length, MFD paths.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

WHERE = ("na", "valid", "lt", "le", "gt", "ge", "eq", "ne", "outlet")          # MHS_PROX_* of the header, then MHS_FLOWPATH_OUTLET
PRODUCTS = ("index", "steps", "dist", "value", "drop")                         # the planes of mhs_flowpath_out, in its order
ROOT_IS_TARGET, NO_LOCAL = 1, 2                                                # the MHS_FLOWPATH_* flags
INT32_MAX = 2 ** 31 - 1


class FlowpathResult(dict):
    """what :func:`flowpath` returns for several products: the planes by name, and ``.info``"""
    info = None


def _check(flowdir, stack, layer, where, threshold, products, value_layer, out_dtype, lonlat, dx, dy):
    """every argument check of :func:`flowpath`, before any device call: (flowdir, where code, threshold, one, names, dx, dy)"""
    import torch
    if isinstance(flowdir, dict):
        if "flowdir" not in flowdir:
            raise ValueError("flowdir: the hydro result holds no 'flowdir' plane; ask hydro for it")
        flowdir = flowdir["flowdir"]
    if not isinstance(flowdir, torch.Tensor) or flowdir.dtype != torch.int8 or flowdir.dim() != 2:
        raise ValueError("flowdir must be a 2-D int8 device tensor or the result of hydro")
    if where not in WHERE:
        raise ValueError(f"unknown where {where!r}: one of {', '.join(WHERE)}")
    code = WHERE.index(where)
    if 2 <= code < 8:
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
    if "value" in names or "drop" in names:
        if value_layer is None:
            raise ValueError("the value and drop products need value_layer, the layer whose values are wanted")
        if not 0 <= int(value_layer) < stack.n_layers:
            raise ValueError(f"value_layer {value_layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1 (index and steps are int32)")
    if tuple(flowdir.shape) != (g.nrow, g.ncol):
        raise ValueError(f"flowdir is {tuple(flowdir.shape)}, the stack's grid ({g.nrow}, {g.ncol})")
    if "dist" in names:
        if lonlat:
            raise ValueError("dist: lonlat=True is out of scope (a cell width per row); bring the raster onto a metric grid with "
                             "resample.resample, or give dx and dy")
        dx = float(g.xres if dx is None else dx)
        dy = float(g.yres if dy is None else dy)
        if not (0.0 < dx < float("inf") and 0.0 < dy < float("inf")):
            raise ValueError("dx and dy must be finite and positive")
    else:
        dx = dy = 0.0
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    return flowdir, code, threshold, one, names, dx, dy


def flowpath(flowdir, stack, layer=0, where="outlet", threshold=None, products=("index",), value_layer=None, root_is_target=True, local=True,
             out_dtype=None, stream=None, lonlat=False, dx=None, dy=None):
    """The first target cell on every cell's own D8 flow path (include/machisplin_hip.h, section "flow paths").  ``flowdir`` is
    an int8 device tensor in the encoding of :func:`terrain.hydro` (0 .. 7 = E, SE, S, SW, W, NW, N, NE, -1 the water leaves, -2
    NA) or the result of ``hydro`` asked for ``flowdir``.  A valid cell is a target when layer ``layer`` of ``stack`` satisfies
    ``where``, one of :data:`WHERE`: the predicates of ``proximity`` (``na``, ``valid``, ``lt le gt ge eq ne`` against
    ``threshold``) or ``outlet``: no targets, the path runs to its root, the cell where the water leaves.  A path that meets
    no target ends at its root when ``root_is_target`` (always, for ``outlet``); otherwise the cell is unreached.

    ``products`` names some of :data:`PRODUCTS`: ``index`` (int32, the cell number row * ncol + col of the path's end; with
    ``outlet`` a catchment label), ``steps`` (int32), ``dist`` (the path's length, a straight step ``dx`` or ``dy`` and a
    diagonal one sqrt(dx^2 + dy^2); the geometry's resolution unless given; refused with ``lonlat=True``), ``value`` (layer
    ``value_layer`` at the path's end) and ``drop`` (that layer at the cell minus at the path's end: the height above the
    drainage when it is the DEM).  Unreached and NA cells are -1 and NaN.  ``local=False`` skips the in-tile phase of the
    doubling (a diagnostic; the planes are the same).  The call synchronises ``stream`` once per doubling round.

    Returns ``(planes, info)``: a dict of device tensors by name (``.info`` too) -- or the single tensor when ``products`` is
    one name -- and a dict of the fields of mhs_flowpath_info (n_valid, n_targets, n_roots, n_unreached, max_steps, rounds,
    scratch_bytes).  MhsError (ERR_INVALID) for a malformed direction plane or one with a cycle."""
    import torch
    flowdir, code, threshold, one, names, dx, dy = _check(flowdir, stack, layer, where, threshold, products, value_layer, out_dtype, lonlat, dx, dy)
    out_dtype = out_dtype or torch.float64
    g = stack.geom
    src = stack.planes
    if flowdir.device != src.device or flowdir.stride(1) != 1:
        flowdir = flowdir.to(src.device).contiguous()
    planes = {n: torch.empty((g.nrow, g.ncol), dtype=torch.int32 if n in ("index", "steps") else out_dtype, device=src.device) for n in names}
    out = _lib.FlowpathOut(*[planes[n].data_ptr() if n in planes else None for n in PRODUCTS])
    info = _lib.FlowpathInfo()
    cg = g.c_struct()
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    cs = _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)
    st = stream if stream is not None else torch.cuda.current_stream(src.device).cuda_stream
    flags = (ROOT_IS_TARGET if root_is_target else 0) | (0 if local else NO_LOCAL)
    _lib.check(_lib.lib().mhs_flowpath_dev(C.byref(cg), flowdir.data_ptr(), flowdir.stride(0), C.byref(cs), int(layer), code, threshold,
                                           int(value_layer) if value_layer is not None else -1, flags, dx, dy, C.byref(out),
                                           _lib.F64 if out_dtype == torch.float64 else _lib.F32, g.ncol, st, C.byref(info)))
    info = {k: getattr(info, k) for k, _ in _lib.FlowpathInfo._fields_}
    if one:
        return planes[names[0]], info
    res = FlowpathResult(planes)
    res.info = info
    return res, info
