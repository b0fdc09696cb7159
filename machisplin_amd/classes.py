"""Categorical layers on the device: class counts, fractions and mode per zone, per coarser cell and per window.

The members take numeric covariates only, so a land-cover raster (NLCD, CORINE, WorldCover, MODIS IGBP) enters a stack as
CLASS FRACTIONS -- the share of forest, water or built-up land in the model cell, within R cells, or in the basin.  What
``terra::crosstab``, ``terra::aggregate(fun = "modal")`` and ``terra::focal`` per class are used for:

* :func:`crosstab` -- the classes inside each zone of an integer zone plane (``zonal``'s missing ``mode``),
* :func:`aggregate` -- the classes inside each cell of another geometry (land cover finer than the model grid),
* :func:`focal` -- the classes within ``radius`` cells of every cell.

include/machisplin_hip.h, section "classes", states the rule: a value is the class ``k`` whose code it equals exactly, every
other valid value is ``other``, and every accumulator is an exact integer count, so no result depends on the order of
addition and every table and plane equals a numpy restatement bit for bit.  A tie of the mode goes to the smaller code.  All
work on the cells runs in libmachisplin_hip.so (csrc/classes.hip); this module only marshals arguments.

Out of scope: the "present" table form, several radii per call, codes outside 0 .. 65 535 or more than 256 classes, Shannon
entropy, area weights on lon/lat grids, a median per zone (:func:`zonal.quantile` has it), more than 2^31 - 1 cells.
"""
from __future__ import annotations

import ctypes as C
import operator

from . import _lib
from .raster import Geometry

MAX_CLASSES = 256
MAX_CODE = 65535
INT32_MAX = 2 ** 31 - 1
TABLE_STATS = ("counts", "n", "other", "cells", "mode", "mode_frac", "variety", "simpson", "frac")
ZONE_PLANES = ("mode", "mode_frac", "variety", "simpson", "n", "frac")
AGGREGATE_PRODUCTS = ("mode", "variety", "n", "mode_frac", "simpson", "frac")
FOCAL_PRODUCTS = ("frac", "mode", "mode_frac", "variety", "n")
SHAPES = ("square", "circle")
_INT = ("counts", "n", "other", "cells", "mode", "variety")


def _names(what, names, allowed):
    names = (names,) if isinstance(names, str) else tuple(names)
    for n in names:
        if n not in allowed:
            raise ValueError(f"unknown name {n!r} in {what}: one of {', '.join(allowed)}")
    if len(set(names)) != len(names):
        raise ValueError(f"{what} must name each of its entries once")
    return names


def _code(what, c):
    """a code of ``classes`` or ``frac_of`` as an int; a value that is no whole number is refused, not truncated"""
    try:
        if int(c) == c:
            return int(c)
    except (TypeError, ValueError, OverflowError):
        pass
    raise ValueError(f"{what} holds {c!r}: a code must be a whole number in 0 .. {MAX_CODE}")


def _codes(classes, frac_of, once=False):
    """the class list (sorted ascending; None: measured) and frac_of, checked: (classes, frac_of)"""
    if classes is not None:
        classes = [_code("classes", c) for c in classes]
        if not 1 <= len(classes) <= MAX_CLASSES:
            raise ValueError(f"classes holds {len(classes)} codes: K must be in 1 .. {MAX_CLASSES}")
        for c in classes:
            if not 0 <= c <= MAX_CODE:
                raise ValueError(f"class code {c} is not in 0 .. {MAX_CODE}")
        if len(set(classes)) != len(classes):
            raise ValueError("classes must hold distinct codes")
        classes = sorted(classes)
    frac_of = tuple(_code("frac_of", c) for c in frac_of)
    for c in frac_of:
        if not 0 <= c <= MAX_CODE:
            raise ValueError(f"frac_of code {c} is not in 0 .. {MAX_CODE}")
        if classes is not None and c not in classes:
            raise ValueError(f"frac_of code {c} is not one of the {len(classes)} classes")
    if once and len(set(frac_of)) != len(frac_of):
        raise ValueError("frac_of must name a code once")
    return classes, frac_of


def _layer(stack, layer, out_dtype):
    import torch
    g = stack.geom
    if not 0 <= int(layer) < stack.n_layers:
        raise ValueError(f"layer {layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1")
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")


def _geometry(which, g):
    """``resample``'s refusals of a grid"""
    import math
    if not isinstance(g, Geometry):
        raise ValueError(f"the {which} geometry must be a Geometry")
    if not (0 < g.nrow < 2 ** 30 and 0 < g.ncol < 2 ** 30):
        raise ValueError(f"bad {which} grid dimension (nrow, ncol must be in 1 .. 2^30)")
    if not (math.isfinite(g.xres) and g.xres > 0 and math.isfinite(g.yres) and g.yres > 0):
        raise ValueError(f"the {which} grid's cell size must be finite and positive")
    if not (math.isfinite(g.xmin) and math.isfinite(g.ymax)):
        raise ValueError(f"the {which} grid's origin must be finite")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"{which} grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1")


def _c_stack(stack):
    import torch
    src = stack.planes
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    return _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)


def _ints(values):
    return (C.c_int32 * len(values))(*values) if values else None


def _info(info):
    d = {k: getattr(info, k) for k, _ in _lib.ClassInfo._fields_ if k != "codes"}
    d["codes"] = [int(info.codes[k]) for k in range(info.K)]
    return d


def measure(stack, layer=0, stream=None):
    """The census of layer ``layer``: a dict of the fields of mhs_class_info -- ``codes`` (the distinct integer values in
    0 .. 65 535 present, ascending; more than 256 is refused with the number found), ``K``, ``n_valid``, ``n_na`` and
    ``n_other`` (valid cells that are no such integer).  What ``classes=None`` does first."""
    import torch
    _layer(stack, layer, None)
    dev = stack.planes.device
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    g, cs, info = stack.geom.c_struct(), _c_stack(stack), _lib.ClassInfo()
    _lib.check(_lib.lib().mhs_class_aggregate_dev(C.byref(g), C.byref(cs), int(layer), C.byref(g), None, 0, None, 0, None, st, C.byref(info)))
    return _info(info)


def _measure_if_sized_by_k(stack, layer, stream, classes, products, frac_of):
    """``classes=None`` costs ONE census: the entry measures the list itself in the census that fills its info.  Only where an
    output is sized by K (``frac`` of all classes) is the list measured beforehand; the call that follows is then given the
    list and asked for no info, and the measuring call's info (None otherwise) is what the caller gets."""
    if classes is not None or "frac" not in products or frac_of:
        return None
    return measure(stack, layer, stream)


def _planes(names, shape, n_frac, out_dtype, dev):
    """the output tensors of a plane-valued call and their struct: (dict, ClassPlanes or None)"""
    import torch
    out = {}
    for n in names:
        if n == "frac":
            out[n] = torch.empty((n_frac,) + shape, dtype=out_dtype, device=dev)
        else:
            out[n] = torch.empty(shape, dtype=torch.int32 if n in _INT else out_dtype, device=dev)
    if not names:
        return out, None
    p = _lib.ClassPlanes()
    for n in names:
        setattr(p, n, out[n].data_ptr())
    p.ld, p.frac_stride = shape[1], shape[0] * shape[1]
    p.dtype = _lib.F64 if out_dtype == torch.float64 else _lib.F32
    return out, p


def crosstab(stack, zones, layer=0, classes=None, n_zones=None, stats=("counts",), planes=(), frac_of=(), out_dtype=None, stream=None):
    """The classes of layer ``layer`` inside each zone of ``zones`` (include/machisplin_hip.h, section "classes"):
    ``terra::crosstab``, and the ``mode`` that ``zonal.zonal`` leaves out.  ``zones`` follows ``zonal.zonal`` exactly: a 2-D
    integer tensor of the stack's ``nrow x ncol``, a negative zone is no zone, a zone ``>= n_zones`` is refused, ``n_zones``
    None is measured.  ``classes`` lists the K <= 256 distinct codes in 0 .. 65 535 (None: the codes present in the layer are
    measured first; more than 256 is refused with the number found); every other valid cell is ``other``.

    ``stats`` names the table's statistics, some of :data:`TABLE_STATS`: ``counts`` (int32, ``n_zones x K``, the columns in
    ascending code), ``n`` (valid cells, ``other`` included), ``other``, ``cells``, ``mode`` (the code with the largest count, the
    SMALLER code on a tie, -1 where no listed class occurs), ``variety`` (int32), ``mode_frac``, ``simpson`` (float64) and
    ``frac`` (float64, ``n_zones x len(frac_of)``; ``frac_of`` empty: all K).  ``planes`` puts some of :data:`ZONE_PLANES` back
    on the cells, float planes of ``out_dtype`` (float64 unless given), ``frac`` as ``(len(frac_of), nrow, ncol)``; -1 or NaN
    where the cell has no zone.  ``n_zones * (K + 3)`` must not pass 2^31 - 1.

    The table is dense: the "present" table form is out of scope, so cell-number labels should be renumbered 0 .. Z - 1 first.
    For ``patches``' ``label`` take its ``id`` plane minus 1.  ``flowpath``'s ``index`` (basins) cannot go through ``patches``:
    basins touch one another, and ``patches`` labels the connected pieces of a mask, so it would merge them; renumber them with
    ``torch.unique(index, return_inverse=True)`` (minus 1 where the plane holds -1).

    Returns ``(table, planes, info)``: two dicts of device tensors by name and a dict of the fields of mhs_class_info
    (K, codes, n_zones, n_valid, n_na, n_other, scratch_bytes)."""
    import torch
    stats = _names("stats", stats, TABLE_STATS)
    planes = _names("planes", planes, ZONE_PLANES)
    if not stats and not planes:
        raise ValueError("no output: stats and planes are both empty")
    classes, frac_of = _codes(classes, frac_of)
    _layer(stack, layer, out_dtype)
    if not isinstance(zones, torch.Tensor) or zones.dim() != 2 or zones.dtype.is_floating_point or zones.dtype.is_complex or zones.dtype == torch.bool:
        raise ValueError("zones must be a 2-D integer tensor (zones given as floats are out of scope)")
    g = stack.geom
    if tuple(zones.shape) != (g.nrow, g.ncol):
        raise ValueError(f"shape mismatch: zones is {tuple(zones.shape)}, the stack's grid ({g.nrow}, {g.ncol})")
    if n_zones is not None:
        n_zones = int(n_zones)
        if not 1 <= n_zones <= INT32_MAX:
            raise ValueError(f"n_zones must be in 1 .. 2^31 - 1 (a zone is an int32), not {n_zones}")
        if classes is not None and n_zones * (len(classes) + 3) > INT32_MAX:
            raise ValueError(f"n_zones * (K + 3) = {n_zones * (len(classes) + 3)} passes 2^31 - 1")
    out_dtype = out_dtype or torch.float64
    src = stack.planes
    dev = src.device
    if zones.device != dev or zones.dtype != torch.int32 or zones.stride(1) != 1:
        zones = zones.to(device=dev, dtype=torch.int32).contiguous()
    cg, cs = g.c_struct(), _c_stack(stack)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    info = _lib.ClassInfo()

    def call(tab, pl, nz, cl):
        _lib.check(_lib.lib().mhs_class_crosstab_dev(C.byref(cg), C.byref(cs), int(layer), zones.data_ptr(), zones.stride(0), nz or 0, _ints(cl),
                                                     len(cl) if cl else 0, _ints(frac_of), len(frac_of), C.byref(tab) if tab is not None else None,
                                                     C.byref(pl) if pl is not None else None, st, C.byref(info)))

    if classes is None or n_zones is None:                      # the library measures the codes and n_zones before the outputs are sized
        call(None, None, n_zones, classes)
        classes, n_zones = [int(info.codes[k]) for k in range(info.K)], info.n_zones
        for c in frac_of:
            if c not in classes:
                raise ValueError(f"frac_of code {c} is not one of the {len(classes)} classes")
    K, n_frac = len(classes), len(frac_of) or len(classes)
    tab_out, tab = {}, None
    if stats:
        rows = max(n_zones, 1)
        width = {"counts": (rows, K), "frac": (rows, n_frac)}
        tab_out = {n: torch.empty(width.get(n, (rows,)), dtype=torch.int32 if n in _INT else torch.float64, device=dev) for n in stats}
        tab = _lib.ClassTable()
        tab.capacity = rows
        for n in stats:
            setattr(tab, n, tab_out[n].data_ptr())
    pl_out, pl = _planes(planes, (g.nrow, g.ncol), n_frac, out_dtype, dev)
    call(tab, pl, n_zones, classes)
    tab_out = {n: v[:n_zones] for n, v in tab_out.items()}
    return tab_out, pl_out, _info(info)


def aggregate(stack, geom, layer=0, classes=None, products=("mode",), frac_of=(), out_dtype=None, stream=None):
    """The classes of layer ``layer`` inside each cell of ``geom``, a grid of the same coordinate system (any resolution,
    origin and extent): ``terra::aggregate(fun = "modal")``, and class cover when land cover is finer than the model grid.  The
    unit of a target cell is the source cells whose centre lies in it -- the footprint of ``resample.resample``'s aggregates,
    so ``n`` is its ``count`` and ``frac`` its ``mean`` of the class's 0 / 1 indicator, bit for bit.  ``products`` names some of
    :data:`AGGREGATE_PRODUCTS`: ``mode variety n`` (int32), ``mode_frac simpson frac`` (``out_dtype``, float64 unless given);
    ``frac`` is ``(len(frac_of), nrow, ncol)``, all K classes when ``frac_of`` is empty.  A target cell with an empty
    footprint (outside the source, or finer than the source) has ``n`` 0, ``mode`` -1 and NaN.

    One target cell's footprint is read by one workgroup: a 1 x 1 target over 10^8 cells is slow -- use :func:`crosstab` with
    one zone for that.

    Returns ``(planes, info)``: a dict of device tensors by name and a dict of the fields of mhs_class_info (where the classes
    are measured for a ``frac`` of all of them, the info is that of the measuring call)."""
    import torch
    products = _names("products", products, AGGREGATE_PRODUCTS)
    if not products:
        raise ValueError("no output: products is empty")
    classes, frac_of = _codes(classes, frac_of)
    _layer(stack, layer, out_dtype)
    _geometry("source", stack.geom)
    _geometry("target", geom)
    out_dtype = out_dtype or torch.float64
    dev = stack.planes.device
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    measured = _measure_if_sized_by_k(stack, layer, st, classes, products, frac_of)
    if measured is not None:
        classes = measured["codes"]
    sg, cs, tg = stack.geom.c_struct(), _c_stack(stack), geom.c_struct()
    out, pl = _planes(products, (geom.nrow, geom.ncol), len(frac_of) or len(classes or ()), out_dtype, dev)
    info = _lib.ClassInfo() if measured is None else None
    _lib.check(_lib.lib().mhs_class_aggregate_dev(C.byref(sg), C.byref(cs), int(layer), C.byref(tg), _ints(classes), len(classes or ()), _ints(frac_of),
                                                  len(frac_of), C.byref(pl), st, C.byref(info) if info is not None else None))
    return out, measured if measured is not None else _info(info)


def focal(stack, radius, layer=0, classes=None, products=("frac",), frac_of=(), shape="square", out_dtype=None, stream=None):
    """The classes of layer ``layer`` in the window of ``radius`` cells (one integer in 1 .. max(nrow, ncol)) around every
    cell: the fraction of a class within R cells.  ``shape`` is ``"square"`` or ``"circle"`` with ``focal.focal``'s windows; NA
    cells and cells outside the raster are skipped, and where the centre is NA every product is NA (-1 for the int32 planes).
    ``products`` names some of :data:`FOCAL_PRODUCTS`: ``frac`` (``(len(frac_of), nrow, ncol)``, all K when ``frac_of`` is
    empty; equal to ``focal.focal`` ``mean`` of the class's indicator at ``offset=0``), ``mode``, ``mode_frac``, ``variety``,
    ``n``.  The cost is one ``focal`` sum per class of the list, whatever ``frac_of``; scratch does not grow with K.

    Returns ``(planes, info)`` as :func:`aggregate` does."""
    import torch
    products = _names("products", products, FOCAL_PRODUCTS)
    if not products:
        raise ValueError("no output: products is empty")
    if shape not in SHAPES:
        raise ValueError(f"unknown shape {shape!r}: one of {', '.join(SHAPES)}")
    classes, frac_of = _codes(classes, frac_of, once=True)
    _layer(stack, layer, out_dtype)
    g = stack.geom
    try:
        radius = operator.index(radius)
    except TypeError:
        radius = 0
    if not 1 <= radius <= max(g.nrow, g.ncol):
        raise ValueError(f"radius must be one integer in 1 .. max(nrow, ncol) = {max(g.nrow, g.ncol)}, got {radius!r}")
    out_dtype = out_dtype or torch.float64
    dev = stack.planes.device
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    measured = _measure_if_sized_by_k(stack, layer, st, classes, products, frac_of)
    if measured is not None:
        classes = measured["codes"]
    cg, cs = g.c_struct(), _c_stack(stack)
    out, pl = _planes(products, (g.nrow, g.ncol), len(frac_of) or len(classes or ()), out_dtype, dev)
    info = _lib.ClassInfo() if measured is None else None
    _lib.check(_lib.lib().mhs_class_focal_dev(C.byref(cg), C.byref(cs), int(layer), radius, SHAPES.index(shape), _ints(classes), len(classes or ()),
                                              _ints(frac_of), len(frac_of), C.byref(pl), st, C.byref(info) if info is not None else None))
    return out, measured if measured is not None else _info(info)
